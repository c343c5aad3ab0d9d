// The arithmetic of a shared instanced scene's update, written ONCE for the host path (instances_shared.hip fill_record / refit_shared_top,
// instances.hip instance_boxes) and the device path (instances_shared_update.hip): an instance's record, its conservative world box, and one
// top-level node over its children's boxes.  Both sides compile with -ffp-contract=off; every operation below is an IEEE fp64 / fp32
// + - * / sqrt, a conversion, a comparison, floor / ceil / ldexp / frexp (exact) or integer work on a float's bits, so host and device produce
// the same bits.  Plain C++ when no HIP compiler is at work (the stand-alone host test includes this file).
#pragma once
#include "bvh.h"
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HR_HD __host__ __device__ inline
#else
#define HR_HD inline
#endif

namespace hr {

// one used slot of a shared scene's top level: topology only (boxes come from a refit)
struct SharedTopNode { int n_internal, n_leaves, child_base, leaf_base, axis, depth; };

namespace imath {

HR_HD double dmin(double a, double b) { return b < a ? b : a; }   // std::min / std::max, spelled out
HR_HD double dmax(double a, double b) { return a < b ? b : a; }
HR_HD float  fmin_(float a, float b) { return b < a ? b : a; }
HR_HD float  fmax_(float a, float b) { return a < b ? b : a; }
HR_HD bool   finite_f(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return (u & 0x7f800000u) != 0x7f800000u; }
HR_HD bool   finite_d(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
HR_HD bool   finite16(const float* m) { bool ok = true; for (int i = 0; i < 16; i++) ok = ok && finite_f(m[i]); return ok; }

// std::nextafter(x, -inf) / (x, +inf) of a float that is not NaN
HR_HD float next_down(float x)
{
    uint32_t u; __builtin_memcpy(&u, &x, 4);
    if ((u << 1) == 0u) u = 0x80000001u;            // +-0 -> the smallest negative subnormal
    else if (u == 0xff800000u) {}                    // -inf stays
    else if (u >> 31) u++; else u--;
    float r; __builtin_memcpy(&r, &u, 4); return r;
}
HR_HD float next_up(float x)
{
    uint32_t u; __builtin_memcpy(&u, &x, 4);
    if ((u << 1) == 0u) u = 0x00000001u;
    else if (u == 0x7f800000u) {}
    else if (u >> 31) u--; else u++;
    float r; __builtin_memcpy(&r, &u, 4); return r;
}

// what the record holds besides the matrix and the fields that never change: the inverse of mat3(m) (adjugate / determinant in double, rounded
// once), the slack terms of the two-level walk (traverse2.h) and the flag that switches object-space culling off.  am: max |p_k| over the mesh's bounds.
HR_HD void record_terms(const float* m, const float* am, float* inv /*[9]*/, float* inv_abs_row /*[3]*/, float* extent_out, uint32_t* flags_out)
{
    double A[3][3];   // A[row][column]
    for (int c = 0; c < 3; c++) for (int q = 0; q < 3; q++) A[q][c] = (double)m[c * 4 + q];
    double C[3][3];   // inverse = adjugate / det
    C[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1]; C[0][1] = A[0][2] * A[2][1] - A[0][1] * A[2][2]; C[0][2] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
    C[1][0] = A[1][2] * A[2][0] - A[1][0] * A[2][2]; C[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0]; C[1][2] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    C[2][0] = A[1][0] * A[2][1] - A[1][1] * A[2][0]; C[2][1] = A[0][1] * A[2][0] - A[0][0] * A[2][1]; C[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    const double det = A[0][0] * C[0][0] + A[0][1] * C[1][0] + A[0][2] * C[2][0];
    bool   ok = det != 0.0 && finite_d(det);
    double norm_a = 0.0, norm_i = 0.0, extent = 0.0;
    for (int q = 0; q < 3; q++)
    {
        double ra = 0.0, ri = 0.0;
        for (int c = 0; c < 3; c++)
        {
            const double v = ok ? C[q][c] / det : 0.0;
            inv[c * 3 + q] = (float)v;
            ok = ok && finite_f(inv[c * 3 + q]);
            ra += __builtin_fabs(A[q][c]); ri += __builtin_fabs(v);
            extent += __builtin_fabs(A[q][c]) * (double)am[c];
        }
        inv_abs_row[q] = (float)(ri * (1.0 + 1e-6));
        extent += __builtin_fabs((double)m[12 + q]);
        norm_a = dmax(norm_a, ra); norm_i = dmax(norm_i, ri);
    }
    float ext = (float)(extent * (1.0 + 1e-6));
    // beyond a condition number of 1e7 the fp32 inverse says little about where the ray is: walk the mesh without culling (slow, rare, correct)
    ok = ok && finite_f(ext) && finite_f(inv_abs_row[0]) && finite_f(inv_abs_row[1]) && finite_f(inv_abs_row[2]) && norm_a * norm_i <= 1e7;
    uint32_t flags = 0u;
    if (!ok)
    {
        for (int q = 0; q < 9; q++) inv[q] = 0.0f;
        inv_abs_row[0] = inv_abs_row[1] = inv_abs_row[2] = 0.0f; ext = 0.0f;
        flags = 1u;
    }
    *extent_out = ext; *flags_out = flags;
}

// conservative world box (lo xyz, hi xyz) of a mesh's object bounds mb (lo > hi: an empty mesh, a point at the instance's origin) under m
HR_HD void world_box(const float* m, const float* mb, float* box /*[6]*/)
{
    double l[3] = { 1e300, 1e300, 1e300 }, h[3] = { -1e300, -1e300, -1e300 };
    if (mb[0] <= mb[3])
        for (int c = 0; c < 8; c++)
        {
            const double x = mb[(c & 1) ? 3 : 0], y = mb[(c & 2) ? 4 : 1], z = mb[(c & 4) ? 5 : 2];
            for (int k = 0; k < 3; k++)
            {
                const double v = (double)m[k] * x + (double)m[4 + k] * y + (double)m[8 + k] * z + (double)m[12 + k];
                const double e = 1e-6 * (__builtin_fabs((double)m[k] * x) + __builtin_fabs((double)m[4 + k] * y) + __builtin_fabs((double)m[8 + k] * z) + __builtin_fabs((double)m[12 + k]));
                l[k] = dmin(l[k], v - e); h[k] = dmax(h[k], v + e);
            }
        }
    else
        for (int k = 0; k < 3; k++) { l[k] = h[k] = (double)m[12 + k]; }
    for (int k = 0; k < 3; k++)
    {
        float lo = (float)l[k], hi = (float)h[k];
        if ((double)lo > l[k]) lo = next_down(lo);
        if ((double)hi < h[k]) hi = next_up(hi);
        box[k] = lo; box[3 + k] = hi;
    }
}

// the pad of every top-level leaf box: 3e-5 x the diagonal of the scene's bounds (bvh_build.cpp: well above the fp32 error of the triangle test)
HR_HD float pad_of_bounds(const float* lo, const float* hi)
{
    const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
    const float  pad = (float)(3e-5 * __builtin_sqrt(dx * dx + dy * dy + dz * dz));
    return pad > 0.0f ? pad : 1e-6f;
}

// The pad of every leaf box of a triangle tree (bvh_build.cpp, refit.h): 3e-5 x the diagonal of the bounds, and never less
// than 2^-21 of the largest coordinate — 4 to 8 float steps there.  A scene that is small against its distance from the origin (a placeholder, a
// collapsed mesh, a mesh that drifted away: diagonal under 1/60 of that distance) has coordinates too coarse to hold 3e-5 diagonals: lo - pad
// would round back to lo, and a ray that runs IN the plane of such a box face meets a slab of no thickness, which the box test rejects.
HR_HD float leaf_pad(const float* lo, const float* hi)
{
    float m = 0.0f;
    for (int k = 0; k < 3; k++) m = fmax_(m, fmax_(__builtin_fabsf(lo[k]), __builtin_fabsf(hi[k])));
    return fmax_(pad_of_bounds(lo, hi), m * 4.76837158203125e-7f);
}

// smallest e in [1, 254] with extent <= 255 * 2^(e - 127) (bvh_build.cpp exponent_for)
HR_HD uint8_t exponent_for(float extent)
{
    if (!(extent > 0.0f)) return 1;
    int ex;
    (void)__builtin_frexpf(extent / 255.0f, &ex);
    int e = ex + 127;
    if (e < 1) e = 1;
    if (e > 254) e = 254;
    while (e > 1 && __builtin_ldexp(255.0, e - 1 - 127) >= (double)extent) e--;
    while (e < 254 && __builtin_ldexp(255.0, e - 127) < (double)extent) e++;
    return (uint8_t)e;
}

HR_HD double half_area3(const float* lo, const float* hi)
{
    const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
    return x * y + y * z + z * x;
}

// One top-level node over its children's boxes (clo / chi: internal children first, then the leaves' padded instance boxes), quantised with the
// builder's rules (lo floored / hi ceiled).  Writes the whole node — counts, child_base, tri_base and meta follow from the topology alone — and its
// own box; returns its half area.
HR_HD double top_node(const SharedTopNode& t, const float (*clo)[3], const float (*chi)[3], Node8& nd, float* lo /*[3]*/, float* hi /*[3]*/)
{
    const int nc = t.n_internal + t.n_leaves;
    const float inf = __builtin_inff();
    for (int k = 0; k < 3; k++) { lo[k] = inf; hi[k] = -inf; }
    for (int c = 0; c < nc; c++)
        for (int k = 0; k < 3; k++) { lo[k] = fmin_(lo[k], clo[c][k]); hi[k] = fmax_(hi[k], chi[c][k]); }
    __builtin_memset(&nd, 0, sizeof(Node8));
    nd.ox = lo[0]; nd.oy = lo[1]; nd.oz = lo[2];
    nd.ex = exponent_for(hi[0] - lo[0]); nd.ey = exponent_for(hi[1] - lo[1]); nd.ez = exponent_for(hi[2] - lo[2]);
    nd.counts = (uint8_t)(t.n_internal | (nc << 4));
    nd.child_base = (uint32_t)t.child_base;
    nd.tri_base = (uint32_t)t.leaf_base;
    const uint8_t eb[3] = { nd.ex, nd.ey, nd.ez };
    for (int c = 0; c < nc; c++)
    {
        // a node without internal children keeps the sort axis out of slot 0's meta byte: a leaf's low bits are its offset
        nd.meta[c] = c < t.n_internal ? (uint8_t)(0x10 | (c == 0 ? t.axis : 0)) : (uint8_t)((1 << 5) | (c - t.n_internal));
        for (int k = 0; k < 3; k++)
        {
            const double sc = __builtin_ldexp(1.0, (int)eb[k] - 127), o = (double)lo[k];
            double l = __builtin_floor(((double)clo[c][k] - o) / sc), h = __builtin_ceil(((double)chi[c][k] - o) / sc);
            if (!(l > 0.0)) l = 0.0;
            if (l > 255.0) l = 255.0;
            if (!(h < 255.0)) h = 255.0;
            if (h < l) h = l;
            nd.qlo[k][c] = (uint8_t)l; nd.qhi[k][c] = (uint8_t)h;
        }
    }
    return half_area3(lo, hi);
}

// ---- the device re-build of a shared scene's top level (instances_shared_rebuild.hip) ---------------------------------------------------------
// The sort key of one instance: a 30-bit Morton code of the centre of its world box inside `bounds` (lo xyz, hi xyz), above the instance index.
// Per axis, all in fp64 (every step one IEEE operation, no contraction):
//     centre = (lo + hi) * 0.5          extent = bounds_hi - bounds_lo          q = ((centre - bounds_lo) / extent) * 1024
//     cell   = floor(q) clamped to [0, 1023]; 0 when q is not finite (a zero extent, an infinite box, 0 / 0)
// x takes bits 0, 3, 6, ..., y bits 1, 4, ..., z bits 2, 5, ...  The key is unique per instance, so the sorted order is a function of the boxes
// and the bounds alone.  An instance of an empty mesh has a point box (world_box) and is sorted by it.
HR_HD uint32_t morton_cell(float lo, float hi, float blo, float bhi)
{
    const double centre = ((double)lo + (double)hi) * 0.5, extent = (double)bhi - (double)blo;
    const double q = ((centre - (double)blo) / extent) * 1024.0;
    if (!finite_d(q)) return 0u;
    const double f = __builtin_floor(q);
    if (!(f > 0.0)) return 0u;
    if (f > 1023.0) return 1023u;
    return (uint32_t)f;
}
HR_HD uint32_t spread3(uint32_t v)   // bit i of a 10-bit value -> bit 3 i
{
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
HR_HD uint32_t morton_code(const float* box /*[6]*/, const float* bounds /*[6]*/)
{
    return spread3(morton_cell(box[0], box[3], bounds[0], bounds[3])) | (spread3(morton_cell(box[1], box[4], bounds[1], bounds[4])) << 1)
         | (spread3(morton_cell(box[2], box[5], bounds[2], bounds[5])) << 2);
}
HR_HD uint64_t sort_key(const float* box, const float* bounds, uint32_t instance) { return ((uint64_t)morton_code(box, bounds) << 32) | (uint64_t)instance; }

// The fixed 8-wide top level over n instances: a shape that depends on n alone.  Leaves 0 .. n-1 are dealt in order to ceil(n / 8) bottom nodes,
// node j of a level of c nodes over m items taking items [floor(j m / c), floor((j + 1) m / c)) — floor or ceil of m / c each, at least 4 when
// m > 8 —; those nodes are grouped the same way until one root stands.  The depth count is the smallest any 8-wide tree over n leaves can have.
// Slots are breadth-first (the root is slot 0, every depth a contiguous range), axis is 0 (the walk's ordering hint only), and a node without
// leaves carries the first leaf below it as leaf_base.
HR_HD int fixed_top_depths(int n) { int d = 1; for (long long c = 8; c < (long long)n; c *= 8) d++; return d; }
HR_HD int fixed_top_level_count(int n, int level) { long long c = n; for (int l = 0; l <= level; l++) c = (c + 7) / 8; return (int)c; }   // level 0: the bottom nodes
HR_HD int fixed_top_nodes(int n) { int s = 0; for (int l = 0; l < fixed_top_depths(n); l++) s += fixed_top_level_count(n, l); return s; }
// first slot of depth d (d == n_depths: the slot count)
HR_HD int fixed_top_depth_start(int n, int d) { const int D = fixed_top_depths(n); int s = 0; for (int k = 0; k < d; k++) s += fixed_top_level_count(n, D - 1 - k); return s; }
// node j of depth d
HR_HD SharedTopNode fixed_top_node(int n, int d, int j)
{
    const int D = fixed_top_depths(n), level = D - 1 - d;
    const long long c = fixed_top_level_count(n, level), m = level == 0 ? n : fixed_top_level_count(n, level - 1);
    const long long first = ((long long)j * m) / c, end = ((long long)(j + 1) * m) / c;
    SharedTopNode t;
    t.axis = 0; t.depth = d;
    if (level == 0) { t.n_internal = 0; t.n_leaves = (int)(end - first); t.child_base = 0; t.leaf_base = (int)first; return t; }
    t.n_internal = (int)(end - first); t.n_leaves = 0; t.child_base = fixed_top_depth_start(n, d + 1) + (int)first;
    long long leaf = first;   // the first leaf below: follow the first child down
    for (int l = level - 1; l >= 0; l--)
    {
        const long long cc = fixed_top_level_count(n, l), mm = l == 0 ? n : fixed_top_level_count(n, l - 1);
        leaf = (leaf * mm) / cc;
    }
    t.leaf_base = (int)leaf;
    return t;
}

} // namespace imath
} // namespace hr
