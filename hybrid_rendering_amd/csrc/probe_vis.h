// Device functions of the probe-grid visualisation (include/hr_probe_vis.h states the contract; probe_vis.hip holds the kernel).
// Everything that decides an output bit is here and is the same code on both paths of the kernel: the sphere test, the order two accepted
// hits are ranked in, the depth test and the colour.  The walks only choose which probes the test sees.
#pragma once
#include "shading.h"

namespace hr {

// the sphere test of the contract — the ONLY place a probe is accepted or refused.  d is unit length.
HR_DEV bool probe_sphere_test(f3 o, f3 d, f3 c, float r, float& t)
{
    const f3    oc   = sub3(o, c);
    const float b    = dot3(oc, d);
    const f3    q    = mk3(oc.x - d.x * b, oc.y - d.y * b, oc.z - d.z * b);
    const float disc = r * r - dot3(q, q);
    if (!(disc >= 0.0f)) return false;   // a NaN: no hit
    t = -b - hr_sqrt(disc);
    return t > 0.0f;                     // front faces in front of the eye
}

struct ProbeHit { float t; int p; };     // p < 0: none
HR_DEV ProbeHit probe_no_hit() { ProbeHit h; h.t = INFINITY; h.p = -1; return h; }

// the probe whose probe_index_to_grid_coord is (cx, cy, cz)
HR_DEV int probe_index_of(const DDGIU& g, int cx, int cy, int cz) { return cx + cy * g.probe_counts[0] + cz * (g.probe_counts[0] * g.probe_counts[1]); }

// test probe (cx, cy, cz) and keep it if it beats `best`: the smaller t, on a tie the smaller index — independent of the order probes arrive in
HR_DEV void probe_consider(const DDGIU& g, f3 o, f3 d, float r, int cx, int cy, int cz, ProbeHit& best)
{
    float t;
    if (!probe_sphere_test(o, d, grid_coord_to_position(g, cx, cy, cz), r, t)) return;
    const int p = probe_index_of(g, cx, cy, cz);
    if (best.p < 0 || t < best.t || (t == best.t && p < best.p)) { best.t = t; best.p = p; }
}

// every probe, in index order: the general path, and what the fast path must equal
HR_DEV ProbeHit probe_walk_all(const DDGIU& g, f3 o, f3 d, float r)
{
    ProbeHit best = probe_no_hit();
    for (int cz = 0; cz < g.probe_counts[2]; cz++)
        for (int cy = 0; cy < g.probe_counts[1]; cy++)
            for (int cx = 0; cx < g.probe_counts[0]; cx++) probe_consider(g, o, d, r, cx, cy, cz, best);
    return best;
}

// ---- the fast path: r <= half the smallest step, finite positive steps (the host decides) -------------------------------------------------
// The ray's bound on every rounding error below: 2^-17 of the sum of the magnitudes that enter a coordinate.  The sphere test itself rounds
// (it accepts or refuses within a few ulp of |o - c| of the true sphere), so the walks are conservative against this bound and not against
// the exact geometry: a candidate too many costs one test, a candidate too few would be a missing sphere.
HR_DEV float probe_walk_slack(const DDGIU& g, f3 o, float r)
{
    float m = r;
#pragma unroll
    for (int a = 0; a < 3; a++) m += fabsf(g.grid_start_position[a]) + fabsf(g.grid_step[a]) * (float)g.probe_counts[a];
    m += (fabsf(o.x) + fabsf(o.y)) + fabsf(o.z);
    return m * 7.62939453125e-6f;   // 2^-17
}

// does the ray (t >= 0) touch the lattice's box grown by half a step (+ slack) on every side?  Conservative: true when in doubt, true for a NaN.
// t_exit: a bound on the parameter at which the ray leaves that box for good — every sphere of the fast path lies inside it
HR_DEV bool probe_ray_hits_box(const DDGIU& g, f3 o, f3 d, float slack, float& t_exit)
{
    const float oo[3] = { o.x, o.y, o.z }, dd[3] = { d.x, d.y, d.z };
    float t0 = 0.0f, t1 = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; a++)
    {
        const float grow = 0.5f * g.grid_step[a] + slack;
        const float lo = g.grid_start_position[a] - grow, hi = (g.grid_step[a] * (float)(g.probe_counts[a] - 1) + g.grid_start_position[a]) + grow;
        if (dd[a] == 0.0f)
        {
            if (oo[a] < lo || oo[a] > hi) return false;
            continue;
        }
        const float ta = __fdiv_rn(lo - oo[a], dd[a]), tb = __fdiv_rn(hi - oo[a], dd[a]);
        const float tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
        if (tn > t0) t0 = tn;
        if (tf < t1) t1 = tf;
    }
    t_exit = t1 + (fabsf(t1) * 1.0e-5f + slack);
    return !(t0 > t_exit);
}

// float -> lattice coordinate that cannot overflow: clamped to [-2, n + 1] as a float first (a NaN: -2)
HR_DEV int probe_coord_clamped(float q, int n)
{
    const float hi = (float)(n + 1);
    return (int)(q > -2.0f ? (q < hi ? q : hi) : -2.0f);
}

// A DDA over the lattice along the ray's major axis k (|d.k| >= 1 / sqrt(3)), one lattice plane per step, nearest plane first.  In plane c the
// ray passes the point Q; a sphere centred in that plane that the ray touches has its centre within r / |d.k| of Q (the centre's distance from
// the LINE is at most r, and the line leaves the plane at an angle whose sine is |d.k|), so on each of the two other axes the candidates are
// the lattice coordinates within r / |d.k| + slack of Q: the cell Q lies in and whichever neighbours that interval reaches — at most 3 x 3,
// usually 2 x 2 or fewer, also for a ray in a cell boundary or with zero components (then Q does not move on that axis).  The walk ends at
// the first plane whose slab [c - r, c + r] the ray enters beyond the best hit, or beyond the point where it leaves the lattice's box: every
// later plane's spheres lie beyond it too.
// inv_step: 1 / grid_step, rounded once (the host's): the quotients below only choose candidates, and what a product with the rounded reciprocal
// is off by — 2^-22 of a lattice coordinate — is inside the slack, which counts the lattice's whole extent
HR_DEV ProbeHit probe_walk_planes(const DDGIU& g, const float* __restrict__ inv_step, f3 o, f3 d, float r, float slack, float t_exit)
{
    ProbeHit best = probe_no_hit();
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const int   k  = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    // the axes in the order (k, k + 1, k + 2): selects, not indexed arrays — nothing of this lives in scratch
#define PV_SEL(v0, v1, v2, a) ((a) == 0 ? (v0) : ((a) == 1 ? (v1) : (v2)))
    const int   j1 = k == 2 ? 0 : k + 1, j2 = k == 0 ? 2 : k - 1;
    const float ok = PV_SEL(o.x, o.y, o.z, k), o1 = PV_SEL(o.x, o.y, o.z, j1), o2 = PV_SEL(o.x, o.y, o.z, j2);
    const float dk = PV_SEL(d.x, d.y, d.z, k), d1 = PV_SEL(d.x, d.y, d.z, j1), d2 = PV_SEL(d.x, d.y, d.z, j2);
    const float sk = PV_SEL(g.grid_start_position[0], g.grid_start_position[1], g.grid_start_position[2], k);
    const float s1 = PV_SEL(g.grid_start_position[0], g.grid_start_position[1], g.grid_start_position[2], j1);
    const float s2 = PV_SEL(g.grid_start_position[0], g.grid_start_position[1], g.grid_start_position[2], j2);
    const float hk = PV_SEL(g.grid_step[0], g.grid_step[1], g.grid_step[2], k);
    const float h1 = PV_SEL(g.grid_step[0], g.grid_step[1], g.grid_step[2], j1);
    const float h2 = PV_SEL(g.grid_step[0], g.grid_step[1], g.grid_step[2], j2);
    const float ik = PV_SEL(inv_step[0], inv_step[1], inv_step[2], k), i1 = PV_SEL(inv_step[0], inv_step[1], inv_step[2], j1), i2 = PV_SEL(inv_step[0], inv_step[1], inv_step[2], j2);
    const int   nk = PV_SEL(g.probe_counts[0], g.probe_counts[1], g.probe_counts[2], k);
    const int   n1 = PV_SEL(g.probe_counts[0], g.probe_counts[1], g.probe_counts[2], j1);
    const int   n2 = PV_SEL(g.probe_counts[0], g.probe_counts[1], g.probe_counts[2], j2);
    if (!(fabsf(dk) >= 0.5f)) return best;   // not a unit vector (a NaN, a zero): the test accepts nothing of such a ray
    const float inv  = __fdiv_rn(1.0f, dk);
    const float reach = r * fabsf(inv) * 1.001f + slack;   // lateral reach in a plane, and the slab's half width in t
    const bool  up   = dk > 0.0f;
    // the first plane that can hold a sphere in front of the eye: the one at or behind the eye, one more for the rounding of the quotient
    // (r <= hk / 2: the plane before that one ends at least r behind the eye)
    const float qk = (ok - sk) * ik;
    int c = up ? probe_coord_clamped(floorf(qk), nk) - 1 : probe_coord_clamped(ceilf(qk), nk) + 1;
    c = up ? (c < 0 ? 0 : c) : (c > nk - 1 ? nk - 1 : c);
    for (; up ? c < nk : c >= 0; c += up ? 1 : -1)
    {
        const float tc = ((hk * (float)c + sk) - ok) * inv;   // the ray's parameter in plane c
        if (tc - reach > (best.p >= 0 && best.t < t_exit ? best.t : t_exit)) break;   // beyond the best hit, or out of the box
        if (tc + reach < 0.0f) continue;                      // the whole slab is behind the eye
        const float q1 = o1 + d1 * tc, q2 = o2 + d2 * tc;
        int lo1 = probe_coord_clamped(floorf(((q1 - reach) - s1) * i1), n1), hi1 = probe_coord_clamped(ceilf(((q1 + reach) - s1) * i1), n1);
        int lo2 = probe_coord_clamped(floorf(((q2 - reach) - s2) * i2), n2), hi2 = probe_coord_clamped(ceilf(((q2 + reach) - s2) * i2), n2);
        lo1 = lo1 < 0 ? 0 : lo1; hi1 = hi1 > n1 - 1 ? n1 - 1 : hi1;
        lo2 = lo2 < 0 ? 0 : lo2; hi2 = hi2 > n2 - 1 ? n2 - 1 : hi2;
        for (int c2 = lo2; c2 <= hi2; c2++)
            for (int c1 = lo1; c1 <= hi1; c1++)
            {
                const int cx = PV_SEL(c, c2, c1, k), cy = PV_SEL(c1, c, c2, k), cz = PV_SEL(c2, c1, c, k);
                probe_consider(g, o, d, r, cx, cy, cz, best);
            }
    }
#undef PV_SEL
    return best;
}

// the winner's depth test: VK_COMPARE_OP_LESS against the G-buffer's depth, in front of the eye
HR_DEV bool probe_depth_test(f3 P, const float* __restrict__ view_proj, float depth_in, float& z)
{
    const f4 clip = mul_m4(view_proj, P.x, P.y, P.z, 1.0f);
    z = __fdiv_rn(clip.z, clip.w);
    return clip.w > 0.0f && z < depth_in;
}

// what == 0: the irradiance atlas at the sphere's normal, as the reference's fragment shader; what == 1: the depth atlas's mean distance / max_distance
HR_DEV uint2 probe_colour(const DDGIU& g, f3 n, int p, int what, const AtlasRGBA& irradiance, const AtlasRG& depth)
{
    float u, v;
    if (what == 0)
    {
        texture_coord_from_direction(n, p, g.irradiance_texture_width, g.irradiance_texture_height, g.irradiance_probe_side_length, u, v);
        const f3 rgb = atlas_bilinear_rgb(irradiance, u, v);
        return make_uint2(pack_h2(rgb.x, rgb.y), pack_h2(rgb.z, 1.0f));
    }
    texture_coord_from_direction(n, p, g.depth_texture_width, g.depth_texture_height, g.depth_probe_side_length, u, v);
    float mean, m2;
    atlas_bilinear_rg(depth, u, v, mean, m2);
    const float gr = __fdiv_rn(mean, g.max_distance);
    return make_uint2(pack_h2(gr, gr), pack_h2(gr, 1.0f));
}

} // namespace hr
