"""CPU only.  The families of tests/shading_cases.py on the oracle's mirror (orc_selftest_shading):
(a) each family reaches what it is named for — asserted on the oracle's own outputs and on the intermediates it records (IrrProbeTrace), so that
    the case file cannot be hollowed out without a test noticing;
(b) the oracle agrees with the plain float64 restatement of tests/shading_reference.py: discrete outputs equal, continuous ones within the bounds
    of tests/golden/shading_layer.json (twice the worst error measured over the bulk families, tools/shading_bounds.py), classes (NaN, inf, finite)
    equal everywhere.  Only a plane whose expected value a constructed tie family writes down itself is not put to the float64 restatement.
tests/test_gpu_shading_layer.py then compares the device with the oracle bit for bit on the same families."""
import json
import os

import numpy as np
import pytest

import shading_cases as sc
import shading_reference as sr

F32 = np.float32
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_layer.json")))


@pytest.fixture(scope="module")
def run(oracle):
    cache = {}

    def go(case, mode=None, inp=None, nout=None):
        key = (id(case), mode, None if inp is None else inp.tobytes())
        if key not in cache:
            cache[key] = oracle.selftest_shading(case.mode if mode is None else mode, case.inp if inp is None else inp, case.tables, case.nout if nout is None else nout)
        return cache[key]
    return go


def _all(mode, name):
    cs = sc.family(mode, name)
    assert cs, (sc.MODE_NAMES[mode], name)
    return cs


# ---------------------------------------------------------------------------------------------------------------- (b) oracle vs float64
@pytest.mark.parametrize("mode", range(12), ids=sc.MODE_NAMES)
def test_oracle_agrees_with_the_float64_restatement(run, mode):
    problems, seen = [], set()
    for c in sc.cases(mode):
        out = run(c)
        for plane, want in c.expect.items():      # a tie family's outcome by the documented priority
            bad = (out[plane].view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(out[plane]) & np.isnan(want))
            if bad.any():
                i = np.flatnonzero(bad)[:3]
                problems.append(f"{c.name} plane {plane}: {int(bad.sum())} off the documented priority, first in {c.inp[i, :9].tolist()} got {out[plane][i]} want {want[i]}")
        for chk in sr.reference(c):
            if set(chk.planes) & set(c.expect):
                continue
            seen.add(chk.function)
            o = out[chk.planes].astype(np.float64)
            cls = (sr.classes(o) != sr.classes(chk.ref)).any(0)
            if cls.any():
                i = np.flatnonzero(cls)[:3]
                problems.append(f"{c.name} {chk.function}: {int(cls.sum())} elements of another class (NaN / inf / finite), first in {c.inp[i, :12].tolist()} oracle {o[:, i].T.tolist()} "
                                f"float64 {chk.ref[:, i].T.tolist()}")
            if chk.discrete:
                bad = ((o != chk.ref) & ~(np.isnan(o) & np.isnan(chk.ref))).any(0)
                if bad.any():
                    i = np.flatnonzero(bad)[:3]
                    problems.append(f"{c.name} {chk.function}: {int(bad.sum())} discrete results differ, first in {c.inp[i, :9].tolist()} oracle {o[:, i].T.tolist()} float64 {chk.ref[:, i].T.tolist()}")
                continue
            e = sr.error_units(out, chk)
            if c.family in GOLDEN["class_only"].get(chk.function, {}).get("families", []):
                unit = np.maximum(sr.ulp32(chk.ref), sr.ULP1 * np.asarray(chk.scale, np.float64))
                with np.errstate(all="ignore"):
                    sign = np.isfinite(e) & (np.abs(o) > unit) & (np.abs(chk.ref) > unit) & (np.signbit(o) != np.signbit(chk.ref))
                if sign.any():
                    problems.append(f"{c.name} {chk.function}: {int(sign.sum())} values of the other sign")
                continue
            bound = GOLDEN["functions"][chk.function]["bound"]
            with np.errstate(all="ignore"):
                over = (e > bound).any(0)
            if over.any():
                i = np.flatnonzero(over)[:3]
                problems.append(f"{c.name} {chk.function}: {int(over.sum())} elements over the bound of {bound} units (worst {np.nanmax(e):.4g}), first in {c.inp[i, :12].tolist()} "
                                f"oracle {o[:, i].T.tolist()} float64 {chk.ref[:, i].T.tolist()}")
    assert seen, "no function of this mode was compared"
    assert not problems, "\n".join(problems)


def test_the_stored_bounds_are_the_measured_ones(oracle):
    """tests/golden/shading_layer.json holds what tools/shading_bounds.py measures today: twice the worst bulk error, for every function"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import shading_bounds
    worst, _ = shading_bounds.measure(oracle)
    assert set(worst) == set(GOLDEN["functions"])
    for f, w in worst.items():
        g = GOLDEN["functions"][f]
        assert abs(g["bulk_worst"] - w) <= 1e-3 * max(w, 1e-12) and abs(g["bound"] - 2 * g["bulk_worst"]) <= 1e-5 * max(g["bound"], 1e-12), (f, w, g)
    assert shading_bounds.CLASS_ONLY == GOLDEN["class_only"]


# ---------------------------------------------------------------------------------------------------------------- (a) the cases reach their edges
def test_cube_family_reaches_faces_edges_corners_and_both_sides(run):
    for S, ps, pl, ls in sc.CUBE_SETS:
        key = sc.cube_tables(S, ps, pl, ls)["key"]
        (faces,), (edges,), (corners,), (nb,) = [sc.family(sc.CUBE, n, key) for n in ("faces", "edge_ties", "corner_ties", "tie_neighbours")]
        assert set(run(faces)[0].astype(int)) == set(range(6))
        d = edges.inp[:, 0:3]
        a = np.abs(d)
        order = np.argsort(-a, axis=1, kind="stable")
        two = np.take_along_axis(a, order, 1)
        assert (two[:, 0] == two[:, 1]).all() and (two[:, 1] > two[:, 2]).all()                   # exactly two equal largest components
        ties = {(tuple(sorted(o[:2])), d[i, sorted(o[:2])[0]] > 0, d[i, sorted(o[:2])[1]] > 0) for i, o in enumerate(order)}
        assert len(ties) == 12
        assert np.array_equal(run(edges)[0], sc.face_by_priority(d))                               # x over y over z, on the oracle
        assert (run(edges)[0] // 2 == np.array([min(sorted(o[:2])) for o in order])).all()        # ... i.e. always the FIRST axis of the pair
        c = corners.inp[:, 0:3]
        assert (np.abs(c[:, 0]) == np.abs(c[:, 1])).all() and (np.abs(c[:, 1]) == np.abs(c[:, 2])).all()
        assert len({tuple(np.sign(r)) for r in c}) == 8 and (run(corners)[0] // 2 == 0).all()
        # one ulp to either side of each tie: the face follows the component that is now larger — both axes of every pair win somewhere
        dirs, side = sc.cube_neighbour_dirs()
        assert np.array_equal(dirs, nb.inp[:, 0:3]) and set(side) == {-1, 1}
        got = run(nb)[0] // 2
        base = sc.cube_edge_dirs()
        for t in range(len(base)):
            pair = sorted(np.argsort(-np.abs(base[t]), kind="stable")[:2])
            assert set(got[4 * t: 4 * t + 4].astype(int)) == set(pair), (base[t], got[4 * t: 4 * t + 4])
        an = np.abs(dirs)
        assert ((np.sort(an, 1)[:, 2] - np.sort(an, 1)[:, 1]) <= np.spacing(np.sort(an, 1)[:, 2])).all()      # really one ulp apart


def test_every_nearest_clamp_is_taken_on_both_ends(run):
    """level and LUT: both clamps; the cube texel: the upper clamp (s * S == S on a face's rim) — the lower one is unreachable, s >= 0 for every
    direction that has a largest component.  Pre-clamp indices in fp32, as the shader forms them; the oracle's fetch returns the clamped texel."""
    for S, ps, pl, ls in sc.CUBE_SETS:
        key = sc.cube_tables(S, ps, pl, ls)["key"]
        (lv,) = sc.family(sc.CUBE, "level_ties", key)
        pre = np.floor((lv.inp[:, 3] + F32(0.5)).astype(F32))
        assert (pre < 0).any() and (pre > pl - 1).any() and all((pre == k).any() for k in range(pl))
        lods = lv.inp[:, 3]
        for k in range(0, pl - 1):      # lod + 0.5 on the integer and an ulp below it: two different levels, one ulp apart
            assert (run(lv)[3][lods == F32(k + 0.5)] == 8 * (k + 1) + 4).all() and (run(lv)[3][lods == sc.up(F32(k + 0.5), -2)] == 8 * k + 4).all()
        (lut,) = sc.family(sc.CUBE, "lut_edges", key)
        for col, plane in ((4, 6), (5, 7)):
            with np.errstate(all="ignore"):
                t = np.floor((lut.inp[:, col] * F32(ls)).astype(F32))
            assert (t < 0).any() and (t > ls - 1).any() and (t == ls).any() and (lut.inp[:, col] == 1).any() and (np.abs(t) >= 2.0 ** 31).any() and np.isnan(t).any()
            got = run(lut)[plane]
            assert (got[t < 0] == 0).all() and (got[t > ls - 1] == ls - 1).all() and (got[np.isnan(t)] == 0).all()
        (rim,) = sc.family(sc.CUBE, "face_rim", key)
        got = run(rim)
        assert (got[2] == S - 1).any() and (got[1] == S - 1).any() and (got[2] == 0).any() and (got[1] == 0).any()
        d = rim.inp[:, 0:3]
        s = (F32(0.5) * ((-d[:, 2] / d[:, 0]).astype(F32) + F32(1))).astype(F32)      # +x face: sc = -z
        assert ((s * F32(S)).astype(F32) == S).any()                                   # the upper clamp itself, not just the last texel


def test_texture_family_wraps_and_leaves_the_int_range(run):
    for t, (w, h) in enumerate(sc.TEX_SIZES):
        (e,) = sc.family(sc.TEXTURE, f"edges_{w}x{h}")
        for col, n in ((1, w), (2, h)):
            i0 = np.floor((e.inp[:, col] * F32(n)).astype(F32) - F32(0.5))
            assert (i0 < 0).any() and (i0 + 1 >= n).any() and (i0 < -n).any() and (i0 >= 2 * n - 1).any(), (w, h, col)       # wraps both ways, more than one period
            assert (i0 == n - 1).any() and (i0 == -1).any()                                                                     # the seam itself: x1 wraps while x0 does not
            assert (e.inp[:, col] == 0).any() and (e.inp[:, col] == 1).any() and (e.inp[:, col] < 0).any() and (e.inp[:, col] == F32(0.5 / n)).any()
        (o,) = sc.family(sc.TEXTURE, f"beyond_int_range_{w}x{h}")
        with np.errstate(all="ignore"):
            px = (o.inp[:, 1] * F32(w)).astype(F32) - F32(0.5)
        assert (px >= 2.0 ** 31).any() and (px <= -2.0 ** 31).any() and np.isnan(px).any() and np.isinf(px).any()
        # the pinned meaning on the oracle: a saturated index, the neighbour taken after the wrap; |px| that large has no fraction, so the result is texel
        # (INT_MAX mod w, y0) or (INT_MIN mod w, y0) itself.  v = 0.3 rows only (a finite, in-range v): compare with the texel row interpolated in y
        tab, data = o.tables["tex_table"], o.tables["tex_data"].view(np.uint8).reshape(-1, 4)
        sel = np.isfinite(px) & (np.abs(px) >= 2.0 ** 31) & (o.inp[:, 2] == F32(0.3)) & (o.inp[:, 0] == t)
        assert sel.any()
        x0 = np.where(px[sel] > 0, sc.INT_MAX % w, (-2 ** 31) % w)
        py = F32(0.3) * F32(h) - F32(0.5)
        y0 = int(np.floor(py)) % h
        fy = F32(py - np.floor(py))
        tex = lambda x, y: (data[int(tab[t][0]) + y * w + x].astype(F32) / F32(255)).astype(F32)
        want = np.array([(tex(x, y0) * (F32(1) - fy) + tex(x, (y0 + 1) % h) * fy).astype(F32) for x in x0])
        assert np.array_equal(run(o)[0:4][:, sel].T, want), (w, h)
    (cut,) = sc.family(sc.TEXTURE, "cutoff_on_a_texel")
    assert set(run(cut)[4]) == {0.0, 1.0}
    bulk = sc.family(sc.TEXTURE, "bulk")[0]
    acc = run(bulk)[4]
    assert 0.05 < acc.mean() < 0.95 and (acc[bulk.inp[:, 3] == 0] == 1).all()      # opaque entries accept, cutout entries do both


def test_lobe_family_sits_on_and_beside_both_basis_thresholds(run):
    n, side, which = sc.threshold_normals()
    (c,) = _all(sc.LOBES, "basis_thresholds")
    assert np.array_equal(np.unique(c.inp[:, 0:3], axis=0), np.unique(n, axis=0))
    for comp, thr in ((1, F32(0.99)), (2, F32(0.999))):
        v = np.abs(n[which == comp][:, comp])
        assert (v < thr).any() and (v == thr).any() and (v > thr).any() and (n[which == comp][:, comp] < 0).any()
        assert (v == sc.up(thr, 1)).any() and (v == sc.up(thr, -1)).any()
    # the threshold is visible in the oracle's output: with |N.y| > 0.99 the basis hangs on (0, 0, 1), so for N = (x, y, 0) the x axis of the basis is
    # cross((0, 0, 1), N) ~ (-y, x, 0) and the lobe's z stays ~0 offset; an ulp below it hangs on (0, 1, 0) and x = cross((0, 1, 0), N) = (0, 0, -x)
    e = sc.lobe_elements(np.array([[np.sqrt(1 - 0.99 ** 2), sc.up(F32(0.99), k), 0] for k in (0, 1)], F32), F32(1e-5), F32(1.0), F32(0.5))
    o = run(c, inp=e)
    # rx = 1e-5: the direction is almost the basis' x axis (sin_theta ~ 1, phi = 2 pi): |z| ~ 1 below the threshold, ~ 0 above it
    assert abs(o[2, 0]) > 0.9 and abs(o[2, 1]) < 0.1 and abs(o[5, 0]) > 0.9 and abs(o[5, 1]) < 0.1
    (r,) = _all(sc.LOBES, "random_number_edges")
    assert (r.inp[:, 3] < F32(1e-5)).any() and (r.inp[:, 3] == F32(1e-5)).any() and (r.inp[:, 4] == 1).any() and (r.inp[:, 3] == 1).any() and (r.inp[:, 3] == 0).any()
    o = run(r)
    below = r.inp[:, 3] < F32(1e-5)
    # under the clamp every rx gives the direction of rx = 1e-5 itself (ry compared by bits: 0 and -0 are two elements)
    on = r.inp[:, 3] == F32(1e-5)
    bits = r.inp[:, 4:6].copy().view(np.uint32)
    for key in {tuple(b) for b in bits[on].tolist()}:
        m = (bits[:, 0] == key[0]) & (bits[:, 1] == key[1])
        ref = o[0:3][:, m & on]
        assert ref.shape[1] == 1 and (m & below).sum() >= 3
        assert (o[0:3][:, m & below].view(np.uint32) == ref.view(np.uint32)).all()


def test_light_family_has_zero_positive_and_non_finite_attenuation(run):
    for mode, plane in ((sc.LIGHT_HARD, 10), (sc.LIGHT_SHADOW, 4)):
        att = np.concatenate([run(c)[plane] for c in sc.cases(mode) if c.family != "bulk"])
        assert (att == 0).any() and (att > 0).any() and (~np.isfinite(att)).any()
        (on,) = _all(mode, "on_the_light")
        t_max = run(on)[9 if mode == sc.LIGHT_HARD else 3]
        assert (t_max[on.inp[:, 19] > 0] == 0).all()                                        # dist == 0
        (cone,) = _all(mode, "spot_cone_ends")
        a = run(cone)[plane]
        d = cone.inp[:, 11 + (0 if mode == sc.LIGHT_SHADOW else 1)]                        # dot(Wi, ldir): one component of ldir
        outer, inner = cone.inp[:, 20], cone.inp[:, 21]
        assert ((d == outer) & (outer < inner)).any() and ((d == inner) & (outer < inner)).any() and (d == sc.up(outer, 1)).any() and (d == sc.up(inner, -1)).any()
        assert (a[(d <= outer) & (outer < inner)] == 0).all() and (a[(d > outer) & (outer < inner)] > 0).all()      # smoothstep 0 on the outer cosine, > 0 an ulp inside
        full = a[(d >= inner) & (outer < inner)]
        assert len(full) and (full == full[0]).all() and (a[(d == sc.up(inner, -1)) & (outer < inner)] <= full[0]).all()
    (par,) = _all(sc.LIGHT_SHADOW, "light_dir_parallel_to_y")
    assert np.isnan(run(par)[0:3]).all()


def _trace(run, case, oracle_mode=12):
    """IrrProbeTrace of all eight probes: [8][12][n]"""
    out = []
    for k in range(8):
        e = case.inp.copy()
        e[:, 11] = k
        out.append(run(case, mode=oracle_mode, inp=e, nout=12))
    return np.array(out)


def test_gather_family_reaches_its_branches(run):
    # all eight probes are one probe
    one = [c for c in sc.family(sc.GATHER, "bulk") if c.tables["counts"] == (1, 1, 1)]
    assert len(one) == 2
    t = _trace(run, one[0])
    assert (t[:, 0:3] == 0).all()
    # a grid with one probe on an axis, P outside the grid, trilinear factors exactly 0 and exactly 1, clamps of the base cell on both ends
    for c in sc.family(sc.GATHER, "on_probes_and_planes") + sc.family(sc.GATHER, "outside_the_grid") + sc.family(sc.GATHER, "beyond_int_range"):
        t = _trace(run, c)
        tri = t[:, 3:6]
        if c.family != "beyond_int_range":
            assert (tri == 0).any() and (tri == 1).any(), c.name
        cnt = np.array(c.tables["counts"])
        f = c.tables["ddgi"].view(F32)
        with np.errstate(all="ignore"):
            cell = ((c.inp[:, 2:5] - f[0:3]) / f[3:6]).astype(F32)
        if c.family == "outside_the_grid":
            assert (cell < 0).any() and (cell > cnt - 1).any()
            for ax in range(3):
                assert (t[0, ax][cell[:, ax] < 0] == 0).all() and (t[7, ax][cell[:, ax] > cnt[ax] - 1] == cnt[ax] - 1).all()
        if c.family == "beyond_int_range":
            assert (np.abs(cell) >= 2.0 ** 31).any() and np.isnan(cell).any()
            big = cell[:, 0] >= 2.0 ** 31
            assert (t[7, 0][big] == cnt[0] - 1).all()                                      # saturated, then clamped to the LAST probe (x86's cast would give the first)
    assert any(c.tables["counts"] == (3, 1, 2) for c in sc.family(sc.GATHER, "bulk"))
    # dist <= mean true and false within an ulp
    (c,) = _all(sc.GATHER, "visibility_one")
    t = _trace(run, c)[0]
    dist, mean = t[6], t[7]
    order = np.argsort(dist)
    le = (dist <= mean)[order]
    flip = np.flatnonzero(le[:-1] & ~le[1:])
    assert len(flip) == 1
    lo, hi = dist[order][flip[0]], dist[order][flip[0] + 1]
    assert hi == np.nextafter(lo, F32(np.inf)) and lo <= mean[order][flip[0]] < hi             # adjacent floats on either side of the mean
    (c,) = _all(sc.GATHER, "visibility_zero")
    t = _trace(run, c)[0]
    assert (t[9] == 0).all() and (t[7] == 0).all()                                              # variance == 0 (mean 0, m2 0)
    (c,) = _all(sc.GATHER, "visibility_m2_below")
    t = _trace(run, c)[0]
    assert (t[7] * t[7] > t[8]).all() and (t[9] > 0).all()                                      # mean^2 > m2: the abs() matters
    # a weight under the 0.2 crush, and one above it
    w = np.concatenate([_trace(run, c)[:, 10].reshape(-1) for c in sc.family(sc.GATHER, "bulk") if c.tables["ddgi"][21] == 1])
    assert (w < 0.2).any() and (w >= 0.2).any() and (w == F32(0.000001)).any()
    w0 = np.concatenate([_trace(run, c)[:, 10].reshape(-1) for c in sc.family(sc.GATHER, "bulk") if c.tables["ddgi"][21] == 0])
    assert (w0 >= 0.2).all()                                                                    # without the visibility test nothing is crushed
    # the net is NaN and 0.5 is returned
    for c in sc.family(sc.GATHER, "nan_net"):
        t = _trace(run, c)[0]
        o = run(c)
        assert (t[11][:2] == 1).all() and (o[5:8][:, :2] == 0.5).all(), c.name
    # every clamp of the bilinear set-up on both ends
    for c in sc.family(sc.GATHER, "bilinear_edges"):
        w, h = int(c.tables["ddgi"][15]), int(c.tables["ddgi"][16])
        with np.errstate(all="ignore"):
            x0 = np.floor((c.inp[:, 0] * F32(w)).astype(F32) - F32(0.5))
            y0 = np.floor((c.inp[:, 1] * F32(h)).astype(F32) - F32(0.5))
        for i0, n in ((x0, w), (y0, h)):
            assert (i0 < 0).any() and (i0 + 1 > n - 1).any() and (i0 > n - 1).any() and (i0 >= 2.0 ** 31).any() and (i0 <= -2.0 ** 31).any() and np.isnan(i0).any()


def test_atlas_extents_above_the_fast_range_are_reached(run):
    (a,) = _all(sc.GI_COORDS, "extent_above_3e5")
    (b,) = _all(sc.GI_COORDS, "extent_above_1e6")
    assert (a.inp[:, 4:6] > 3e5).any() and (a.inp[:, 4:6].max() <= 1e6) and (run(a)[6] == 0).any() and (run(a)[6] == 1).any()
    assert (b.inp[:, 4:6] > 1e6).any() and (run(b)[6] == 0).all()
    assert (run(sc.family(sc.GI_COORDS, "bulk")[0])[6] == 1).all()


def test_surface_family_takes_every_path(run):
    T = sc.surface_tables()
    (z,) = _all(sc.SURFACE, "zero_area_normal")
    assert np.isnan(run(z)[3:6]).all()
    (z,) = _all(sc.SURFACE, "zero_area_triangle")
    assert np.isnan(run(z)[3:6]).all()
    (a,) = _all(sc.SURFACE, "vertex_normals")
    (b,) = _all(sc.SURFACE, "cross_product")
    na, nb = run(a)[3:6][:, a.inp[:, 3] == 1], run(b)[3:6][:, b.inp[:, 3] == 0]
    assert np.isfinite(na).all() and np.isfinite(nb).all() and not np.allclose(na, nb[:, : na.shape[1]], atol=1e-3)
    assert np.allclose(nb, nb[:, :1], atol=1e-6)                                                # the geometric normal does not depend on the barycentrics
    (m,) = _all(sc.SURFACE, "normal_map_tangent_parallel")
    o = run(m)
    assert np.isfinite(o[3:6]).all()
    assert np.array_equal(T["tangents"][4], T["normals"][4])
    tang = o[3:6][:, m.inp[:, 3] == (1 | 4 | 8)]
    plain = run(m, inp=np.where(np.arange(24) == 3, F32(1), m.inp[m.inp[:, 3] == (1 | 4 | 8)]).astype(F32))[3:6]
    cosang = np.abs((tang * plain).sum(0))
    assert (cosang > 1 - 1e-5).all()                                                            # TBN = (T, T, N) with T parallel to N: the mapped normal stays on N's line
    (i,) = _all(sc.SURFACE, "instance_nonuniform_scale")
    o = run(i)
    no_inst = run(i, inp=np.where(np.arange(24) == 3, F32(1), i.inp[i.inp[:, 3] == 3]).astype(F32))
    assert not np.allclose(o[3:6][:, i.inp[:, 3] == 3], no_inst[3:6], atol=1e-2) and np.allclose(np.linalg.norm(o[3:6], axis=0), 1, atol=1e-5)
    assert (run(sc.family(sc.SURFACE, "bulk")[0])[9] >= F32(0.1)).all()                           # the roughness floor
    assert (run(a)[9][a.inp[:, 3] == 1] == F32(0.1)).all()                                      # material 0: roughness 0.05, raised to the floor


def test_brdf_family_puts_every_dot_on_zero_and_the_roughness_on_its_floor(run):
    for mode in (sc.BRDF_TERMS, sc.BRDF_UBER):
        (c,) = _all(mode, "dots_at_zero")
        for col in (19, 20, 21, 22):
            assert (c.inp[:, col] == 0).any() and (c.inp[:, col] == 1).any()
        for col in (20, 21):      # NdotL, NdotV: the products in the denominators, also on -0
            assert np.signbit(c.inp[:, col][c.inp[:, col] == 0]).any()
        assert (c.inp[:, 18] == F32(0.1)).any() and (c.inp[:, 18] == 0).any()
        assert np.isfinite(run(c)).all()                                                        # the EPSILON clamps hold: no 0 / 0
    (o,) = _all(sc.BRDF_UBER, "wo_opposes_wi")
    assert np.isnan(o.inp[:, 9:12]).all() and (o.inp[:, 3:6] == -o.inp[:, 6:9]).all()
    (g,) = _all(sc.BRDF_UBER, "grazing")
    ndl = (g.inp[:, 0:3] * g.inp[:, 6:9]).sum(1)
    ndv = (g.inp[:, 0:3] * g.inp[:, 3:6]).sum(1)
    assert (ndl == 0).any() and (ndv == 0).any() and (ndl < 0).any() and (ndv < 0).any()
