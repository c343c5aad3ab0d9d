// The bottom-up refit of one 8-wide node, shared by the instanced scenes (instances.hip: subtrees under moving matrices, leaves cut to their
// object-space cells) and the refit of split-free trees under new vertices (deform_refit.hip, for the flat deformable scenes of deform.hip and the
// deforming meshes of instances_shared_deform.hip: no instance, no cells, no dirty filter).  A thread recomputes the boxes
// of the node's eight children (internal children: the box their own thread stored one launch — or one barrier — earlier; leaves: the bounds of
// their triangles plus the pad), the node's origin / scale exponents, and requantises: the encoding rules of bvh_build.cpp, in double like there.
//
// Split-free trees under new vertices (kInstanced = false) follow two more of the builder's rules, so that hostile vertex streams keep the answers:
//   * a triangle with a NaN or infinite coordinate has no box (the builder gives it no reference).  A leaf with no finite triangle, and a node
//     with no non-empty child, is EMPTY: its node_box is lo = +inf, hi = -inf, it does not enter its parent's bounds, and its slot is stored
//     INVERTED on all three axes (qlo = 255, qhi = 0).  test_node's slab test then finds the near plane 255 grid steps behind the far plane and
//     rejects the slot for every ray whose origin is nearer than about 2e6 node extents (the far-plane scale 1.0000005 is the only slack); a ray
//     from farther away may enter and finds only triangles the watertight test rejects (tests/test_deform_cases.py pins that).  A node
//     with no finite triangle beneath it keeps origin 0 and exponents 1, the builder's empty node.
//   * the pad is the builder's for the CURRENT vertices: instance_math.h leaf_pad of the exact bounds of the mesh's finite triangles (3e-5 x their
//     diagonal, at least 2^-21 of the largest coordinate, 1e-6 when there are none), from the bounds deform_refit.hip's k_deform_bounds reduced
//     on the same stream just before (the pad stands two orders above the box test's error at every size and place the
//     mesh takes, not only the one it was created with).
// The pad word of a node_box row (index 3) is 0, or NaN when a non-finite triangle lies beneath the node: hr_scene_update_meshes reads the root's.
#pragma once
#include "bvh.h"
#include "instance_math.h"
#include <hip/hip_runtime.h>
#include <cmath>

namespace hr {

struct RefitArgs
{
    Node8*             nodes;
    const TriGPU*      tris;
    float*             node_box;     // [n_nodes][8]: lo xyz, pad, hi xyz, pad
    const uint32_t*    list;         // the nodes of this level
    const float*       cells;        // [n_nodes][8][6]: object-space cell of every LEAF slot (the builder's box of it), lo xyz hi xyz
    const int32_t*     node_inst;    // instance a node belongs to, -1: top level
    const InstanceRec* inst;
    const uint32_t*    dirty;        // per instance: matrix changed in this update
    int                count;
    float              pad;          // of the leaf boxes (deform_refit.hip: refit_pad of the mesh's CURRENT bounds, once per workgroup)
};

// ordered-integer image of a float: unsigned comparison == float comparison
__device__ inline uint32_t ordered_bits(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float ordered_float_dev(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// bvh_build.cpp's pad for bounds reduced by atomicMin / atomicMax from 0xffffffff / 0 (no finite triangle: the builder's zero box)
__device__ inline float refit_pad(const uint32_t* bits)
{
    float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
    if (bits[0] <= bits[3])
        for (int k = 0; k < 3; k++) { lo[k] = ordered_float_dev(bits[k]); hi[k] = ordered_float_dev(bits[3 + k]); }
    return imath::leaf_pad(lo, hi);
}
__device__ inline bool finite_tri(const TriGPU& tr)
{
    bool f = true;
    for (int k = 0; k < 3; k++) f = f && fabsf(tr.v0[k]) < INFINITY && fabsf(tr.v1[k]) < INFINITY && fabsf(tr.v2[k]) < INFINITY;
    return f;
}

__device__ inline uint8_t exponent_for_dev(float extent)
{
    // smallest e with extent <= 255 * 2^(e - 127) (bvh_build.cpp exponent_for; the answer is unique, so the starting guess is free)
    if (!(extent > 0.0f)) return 1;
    int e = (int)((__float_as_uint(extent) >> 23) & 0xffu) - 7;
    if (e < 1) e = 1;
    if (e > 254) e = 254;
    while (e > 1 && ldexp(255.0, e - 1 - 127) >= (double)extent) e--;
    while (e < 254 && ldexp(255.0, e - 127) < (double)extent) e++;
    return (uint8_t)e;
}
__device__ inline float round_down(double v) { float f = (float)v; return (double)f > v ? nextafterf(f, -INFINITY) : f; }
__device__ inline float round_up(double v) { float f = (float)v; return (double)f < v ? nextafterf(f, INFINITY) : f; }

// kInstanced = false: every node is refitted and a leaf's box is the bounds of its triangles (node_inst, cells, inst and dirty are not read).
// Returns the half area of the node's box (what the deformable scenes' refit cost sums; the instanced path ignores it).
template <bool kInstanced>
__device__ inline double refit_node(const RefitArgs& a, const uint32_t ni)
{
    const int      in = kInstanced ? a.node_inst[ni] : -1;
    if (in >= 0 && !a.dirty[in]) return 0.0;   // the instance did not move: its subtree stands
    Node8 n = a.nodes[ni];
    const float pad = a.pad;
    uint32_t empty = 0u;      // bit c: child c holds no finite triangle (never set when kInstanced)
    bool     poisoned = false;   // a non-finite triangle beneath this node
    const int n_internal = n.counts & 15, n_children = n.counts >> 4;
    float clo[8][3], chi[8][3];
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int c = 0; c < n_children; c++)
    {
        if (c < n_internal)
        {
            const float* b = a.node_box + (size_t)(n.child_base + c) * 8;
            for (int k = 0; k < 3; k++) { clo[c][k] = b[k]; chi[c][k] = b[4 + k]; }
            if (!kInstanced) { poisoned = poisoned || b[3] != b[3]; if (!(b[0] <= b[4])) empty |= 1u << c; }
        }
        else
        {
            const uint32_t m = n.meta[c], cnt = m >> 5, off = m & 31u;
            float l[3] = { INFINITY, INFINITY, INFINITY }, h[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (uint32_t t = 0; t < cnt; t++)
            {
                const TriGPU& tr = a.tris[n.tri_base + off + t];
                if (!kInstanced && !finite_tri(tr)) { poisoned = true; continue; }   // (a branch: selects here measured 60 us slower per update)
                for (int k = 0; k < 3; k++)
                {
                    l[k] = fminf(l[k], fminf(tr.v0[k], fminf(tr.v1[k], tr.v2[k])));
                    h[k] = fmaxf(h[k], fmaxf(tr.v0[k], fmaxf(tr.v1[k], tr.v2[k])));
                }
            }
            if (in >= 0)
            {
                // the leaf's object-space cell through the instance's matrix: centre c' = M c, half extent e' = |mat3(M)| e, rounded outwards
                const float*       cell = a.cells + ((size_t)ni * 8 + c) * 6;
                const float*       M    = a.inst[in].m;
                const double cx = 0.5 * ((double)cell[0] + cell[3]), cy = 0.5 * ((double)cell[1] + cell[4]), cz = 0.5 * ((double)cell[2] + cell[5]);
                const double ex = 0.5 * ((double)cell[3] - cell[0]), ey = 0.5 * ((double)cell[4] - cell[1]), ez = 0.5 * ((double)cell[5] - cell[2]);
                for (int k = 0; k < 3; k++)
                {
                    const double wc = ((double)M[k] * cx + (double)M[4 + k] * cy) + ((double)M[8 + k] * cz + (double)M[12 + k]);
                    const double we = (fabs((double)M[k]) * ex + fabs((double)M[4 + k]) * ey) + fabs((double)M[8 + k]) * ez;
                    const double sl = 1e-12 * (fabs(wc) + we);   // the double arithmetic's own rounding, generously
                    l[k] = fmaxf(l[k], round_down(wc - we - sl));
                    h[k] = fminf(h[k], round_up(wc + we + sl));
                }
            }
            if (!kInstanced && !(l[0] <= h[0])) empty |= 1u << c;   // no finite triangle: the bounds stand at +inf / -inf
            for (int k = 0; k < 3; k++)
            {
                if (h[k] < l[k] && !(empty >> c & 1u)) h[k] = l[k];   // (cell and triangles disjoint up to rounding: cannot happen for a builder cell, harmless if it did)
                clo[c][k] = l[k] - pad; chi[c][k] = h[k] + pad;   // bvh_build.cpp finalise(pad)
            }
        }
        if (!(empty >> c & 1u))
            for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], clo[c][k]); hi[k] = fmaxf(hi[k], chi[c][k]); }
    }
    const bool none = n_children == 0 || (!kInstanced && empty == (1u << n_children) - 1u);
    float* nb = a.node_box + (size_t)ni * 8;
    const float flag = poisoned ? __uint_as_float(0x7fc00000u) : 0.0f;
    // an empty node's box stays at +inf / -inf for its parent; a node without children (the builder's, of a scene without triangles) has the zero box
    if (n_children == 0) { for (int k = 0; k < 3; k++) { lo[k] = 0.0f; hi[k] = 0.0f; } }
    nb[0] = lo[0]; nb[1] = lo[1]; nb[2] = lo[2]; nb[3] = flag; nb[4] = hi[0]; nb[5] = hi[1]; nb[6] = hi[2]; nb[7] = 0.0f;
    if (none) { for (int k = 0; k < 3; k++) { lo[k] = 0.0f; hi[k] = 0.0f; } }
    n.ox = lo[0]; n.oy = lo[1]; n.oz = lo[2];
    n.ex = exponent_for_dev(hi[0] - lo[0]); n.ey = exponent_for_dev(hi[1] - lo[1]); n.ez = exponent_for_dev(hi[2] - lo[2]);
    const uint8_t eb[3] = { n.ex, n.ey, n.ez };
    for (int c = 0; c < 8; c++)
        for (int k = 0; k < 3; k++)
        {
            uint8_t ql = 0, qh = 0;
            if (c < n_children && (empty >> c & 1u)) { ql = 255; qh = 0; }   // inverted: no ray enters (see the header)
            else if (c < n_children)
            {
                // child box = origin + q * 2^(e - 127), lo floored / hi ceiled => conservative (bvh.h)
                const double s = ldexp(1.0, (int)eb[k] - 127), o = (double)lo[k];
                double l = floor(((double)clo[c][k] - o) / s), h = ceil(((double)chi[c][k] - o) / s);
                if (!(l > 0.0)) l = 0.0;
                if (l > 255.0) l = 255.0;
                if (!(h < 255.0)) h = 255.0;
                if (h < l) h = l;
                ql = (uint8_t)l; qh = (uint8_t)h;
            }
            n.qlo[k][c] = ql; n.qhi[k][c] = qh;
        }
    a.nodes[ni] = n;
    const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
    return x * y + y * z + z * x;
}

} // namespace hr
