// Two-level walk of a SHARED instanced scene (instances_shared.hip): a top level over the instances' world boxes whose leaves name
// instances, and ONE object-space tree per mesh that every instance of the mesh walks.  One ray per lane, one stack for both levels.
//
// What decides a hit is unchanged (traverse.h): the watertight test on the WORLD-space vertices
// model_matrix * (p, 1) — rounded operation by operation like k_instances_transform — with the WORLD-space ray; the three vertices of a leaf
// triangle are transformed on the fly.  Only the box culling inside an instance runs in object space: the ray enters as
// o' = inv * (o - translation), d' = inv * d (not normalised: t is the same parameter in both spaces, so t_min / t_max and the closest-hit
// shrink carry over), and every slab is widened by a per-(ray, instance) slack, because nothing makes the object-space boxes monotonic
// with the world-space vertex subtraction the way the single-level walk's boxes are.
//
// The slack (shared instanced scenes).  u = 2^-24.  With W = |o - b|_1 + extent (extent bounds |b|_1 + the instance's
// world size), every error that separates "the test accepts the world triangle at parameter t" from "the computed object-space ray is
// inside the triangle's leaf box at t" is a world-space displacement of at most c u W: the rounding of the vertices M p (3 u), of o - b (1 u), of
// inv's entries and of the two 3x3 products (5 u for o', 4 u for d', which acts over |t d| <= |o - b| + size, so twice), the slab arithmetic
// (4 u of |plane - o'|) and the watertight test's own decision error (about 12 u of |v - o|): 33 u together.  A world displacement e moves
// object coordinate k by at most e * sum_j |inv(k, j)|.  Hence slack_k = kSlackU * W * inv_abs_row[k] with kSlackU = 128 u = 2^-17, four
// times the sum.  An instance whose matrix has no safe inverse is walked with infinite slack: every occupied child counts as hit.  The 1e-18
// clamp of d' is outside that sum; boxray_object below says when it matters and what happens then.
#pragma once
#include "traverse.h"

namespace hr {

#ifndef HR_SHARED_SLACK
#define HR_SHARED_SLACK 7.62939453125e-6f   // 2^-17 = 128 u.  Developer self-check: -DHR_SHARED_SLACK=0.0f must fail tests/test_gpu_instances_shared.py's edge test
#endif

// the box-test side of a ray, in the space of the level being walked; w* = slack * |1 / d| widens every slab
struct BoxRay
{
    f3       o;
    float    idx, idy, idz;
    float    wx, wy, wz;
    uint32_t sel;
    uint32_t keep;   // 0xff, or 0 inside an instance whose mask rejects the ray (enter_instance): test_node2 then reports no child hit
};

HR_DEV void boxray_world(BoxRay& b, const RayPre& r)
{
    b.o = r.o; b.idx = r.idx; b.idy = r.idy; b.idz = r.idz; b.sel = r.sel;
    b.wx = 0.0f; b.wy = 0.0f; b.wz = 0.0f;
    b.keep = 0xffu;
}

// HR_SHARED_CLAMP_REACH: a component of d' below the 1e-18 clamp is replaced by it, which moves the computed ray by up to t * 1e-18 object units along
// that axis; a hit lies at t <= W / max|d| (world), so the slack 2^-17 W row_k covers the clamp iff row_k * max|d| >= 1e-18 * 2^17 = 1.3e-13.
// Below that (scales beyond ~1e13, or very short unnormalised directions) a clamped axis is taken out of the slab test.
#define HR_SHARED_CLAMP_REACH 2.0e-13f
HR_DEV void boxray_object(BoxRay& b, f3 o, f3 d, f3 slack, f3 reach, bool no_cull)
{
    b.o = o;
    const float tiny = 1e-18f;   // traverse.h ray_prepare
    const float dx_ = fabsf(d.x) < tiny ? (d.x < 0.0f ? -tiny : tiny) : d.x;
    const float dy_ = fabsf(d.y) < tiny ? (d.y < 0.0f ? -tiny : tiny) : d.y;
    const float dz_ = fabsf(d.z) < tiny ? (d.z < 0.0f ? -tiny : tiny) : d.z;
    b.idx = __builtin_amdgcn_rcpf(dx_); b.idy = __builtin_amdgcn_rcpf(dy_); b.idz = __builtin_amdgcn_rcpf(dz_);
    b.sel = (dx_ < 0.0f ? 1u : 0u) | (dy_ < 0.0f ? 2u : 0u) | (dz_ < 0.0f ? 4u : 0u);
    // reach_k = inv_abs_row[k] * max|d_world|
    b.wx = (no_cull || (fabsf(d.x) < tiny && !(reach.x >= HR_SHARED_CLAMP_REACH))) ? INFINITY : slack.x * fabsf(b.idx);
    b.wy = (no_cull || (fabsf(d.y) < tiny && !(reach.y >= HR_SHARED_CLAMP_REACH))) ? INFINITY : slack.y * fabsf(b.idy);
    b.wz = (no_cull || (fabsf(d.z) < tiny && !(reach.z >= HR_SHARED_CLAMP_REACH))) ? INFINITY : slack.z * fabsf(b.idz);
}

// test_node (traverse.h) with every slab widened by the ray's slack: near planes move by -w, far planes by +w.  w = 0 gives test_node's bits;
// w = inf (or a NaN from inf * 0: fmaxf / fminf drop it) takes the axis out of the test, so every occupied child is hit.
template <int ORDER>
HR_DEV NodeHits test_node2(const NodeRaw& n, const BoxRay& r, float t_near, float t_far)
{
    const uint4 q0 = n.q0, q1 = n.q1, q2 = n.q2, q3 = n.q3, q4 = n.q4;
    const float  nox = __uint_as_float(q0.x), noy = __uint_as_float(q0.y), noz = __uint_as_float(q0.z);
    const float  sx = __uint_as_float((q0.w & 0xffu) << 23), sy = __uint_as_float(((q0.w >> 8) & 0xffu) << 23), sz = __uint_as_float(((q0.w >> 16) & 0xffu) << 23);
    const float  ax = sx * r.idx, ay = sy * r.idy, az = sz * r.idz;
    const float  bx = (nox - r.o.x) * r.idx, by = (noy - r.o.y) * r.idy, bz = (noz - r.o.z) * r.idz;
    const float  bnx = bx - r.wx, bny = by - r.wy, bnz = bz - r.wz, bfx = bx + r.wx, bfy = by + r.wy, bfz = bz + r.wz;
    const bool   nx = r.sel & 1u, ny = r.sel & 2u, nz = r.sel & 4u;
    const uint32_t lox0 = q2.x, lox1 = q2.y, loy0 = q2.z, loy1 = q2.w, loz0 = q3.x, loz1 = q3.y;
    const uint32_t hix0 = q3.z, hix1 = q3.w, hiy0 = q4.x, hiy1 = q4.y, hiz0 = q4.z, hiz1 = q4.w;
    const uint32_t nX[2] = { nx ? hix0 : lox0, nx ? hix1 : lox1 }, fX[2] = { nx ? lox0 : hix0, nx ? lox1 : hix1 };
    const uint32_t nY[2] = { ny ? hiy0 : loy0, ny ? hiy1 : loy1 }, fY[2] = { ny ? loy0 : hiy0, ny ? loy1 : hiy1 };
    const uint32_t nZ[2] = { nz ? hiz0 : loz0, nz ? hiz1 : loz1 }, fZ[2] = { nz ? loz0 : hiz0, nz ? loz1 : hiz1 };
    NodeHits h;
    h.child_base = q1.x; h.tri_base = q1.y; h.meta_lo = q1.z; h.meta_hi = q1.w;
    h.n_internal = (q0.w >> 24) & 15u;
    h.rev = 0u;
    if (ORDER != HR_ORDER_SLOTS)
    {
        const uint32_t along = (r.sel >> (q1.z & 3u)) & 1u;
        h.rev = ORDER == HR_ORDER_NEAR ? along : along ^ 1u;
    }
    uint32_t hits = 0;
#pragma unroll
    for (int half = 0; half < 2; half++)
    {
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const float tnx = hr_fma(ubyte(nX[half], k), ax, bnx), tfx = hr_fma(ubyte(fX[half], k), ax, bfx);
            const float tny = hr_fma(ubyte(nY[half], k), ay, bny), tfy = hr_fma(ubyte(fY[half], k), ay, bfy);
            const float tnz = hr_fma(ubyte(nZ[half], k), az, bnz), tfz = hr_fma(ubyte(fZ[half], k), az, bfz);
            const float tn = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, t_near));
            const float tf = fminf(fminf(tfx, tfy), fminf(tfz, t_far)) * 1.0000005f;
            hits |= (tn <= tf) ? (1u << (half * 4 + k)) : 0u;
        }
    }
    h.hit8 = hits & ((1u << (q0.w >> 28)) - 1u) & r.keep;
    return h;
}

// the part of an instance record the walk keeps while it is inside the instance
struct InstanceIn
{
    float    m[12];   // columns 0..3, rows x y z
    uint32_t first_tri;
    uint32_t mesh_tri_base;   // the attribute index of the mesh's first triangle: what cutout_accept is keyed on (read by CUTOUT walks only)
};

// matrix and first_tri of record `slot` (quads 0..3 and 7 of the record); returns quad 7: extent, flags, first_tri
HR_DEV uint4 load_instance_in(const InstanceShared* __restrict__ inst, uint32_t slot, InstanceIn& in)
{
    const uint4* p = reinterpret_cast<const uint4*>(inst + slot);
    const uint4 c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3], i3 = p[7];
    in.m[0] = __uint_as_float(c0.x); in.m[1] = __uint_as_float(c0.y); in.m[2]  = __uint_as_float(c0.z);
    in.m[3] = __uint_as_float(c1.x); in.m[4] = __uint_as_float(c1.y); in.m[5]  = __uint_as_float(c1.z);
    in.m[6] = __uint_as_float(c2.x); in.m[7] = __uint_as_float(c2.y); in.m[8]  = __uint_as_float(c2.z);
    in.m[9] = __uint_as_float(c3.x); in.m[10] = __uint_as_float(c3.y); in.m[11] = __uint_as_float(c3.z);
    in.first_tri = i3.z; in.mesh_tri_base = i3.w;
    return i3;
}

// Instance masks (hr_scene_set_instance_masks / hr_scene_set_cull_mask; Vulkan's rule): a ray walks into an instance iff the instance's mask — bits
// 8..15 of the record's flags, in quad 7, which the entry holds anyway — and the ray's cull mask (Scene2::cull, shifted to the same bits) share a
// bit.  A rejected instance does not exist for the ray.  The rejection is DATA, not control flow: the entry clears BoxRay::keep, the test of the
// mesh's root node then reports no child hit, and both walks leave the instance through the path they take after any instance they have walked
// to the end — their state machines (the entries parked under sp_base in trace2; the ballot, append and flush section that every lane of
// trace_coop2 executes each iteration) are the ones of a scene without masks.  A rejected instance costs its record and one node test; a branch
// at the entry instead saves that node and costs the trace kernels 3 to 13 % of their time when nothing is masked (docs/EXPERIMENTS.md,
// "Instance masks").  All-0xFF masks, the default, reject nothing and change no bit of any answer.

// loads record `slot`, moves the box-test ray into the instance's object space, returns the mesh root
HR_DEV uint32_t enter_instance(const Scene2& sc, uint32_t slot, f3 o, f3 d, InstanceIn& in, BoxRay& b)
{
    const InstanceShared* __restrict__ inst = sc.inst;
    const uint4  i3 = load_instance_in(inst, slot, in);
    const uint4* p  = reinterpret_cast<const uint4*>(inst + slot);
    const uint4  i0 = p[4], i1 = p[5], i2 = p[6], i4 = p[8];
    const float v00 = __uint_as_float(i0.x), v10 = __uint_as_float(i0.y), v20 = __uint_as_float(i0.z);   // inv, column 0
    const float v01 = __uint_as_float(i0.w), v11 = __uint_as_float(i1.x), v21 = __uint_as_float(i1.y);   // column 1
    const float v02 = __uint_as_float(i1.z), v12 = __uint_as_float(i1.w), v22 = __uint_as_float(i2.x);   // column 2
    const f3    nrm = mk3(__uint_as_float(i2.y), __uint_as_float(i2.z), __uint_as_float(i2.w));
    const float extent = __uint_as_float(i3.x);
    const bool  no_cull = (i3.y & 1u) != 0u;
    const f3 ow = mk3(o.x - in.m[9], o.y - in.m[10], o.z - in.m[11]);
    const f3 oo = mk3((v00 * ow.x + v01 * ow.y) + v02 * ow.z, (v10 * ow.x + v11 * ow.y) + v12 * ow.z, (v20 * ow.x + v21 * ow.y) + v22 * ow.z);
    const f3 od = mk3((v00 * d.x + v01 * d.y) + v02 * d.z, (v10 * d.x + v11 * d.y) + v12 * d.z, (v20 * d.x + v21 * d.y) + v22 * d.z);
    const float W = HR_SHARED_SLACK * (((fabsf(ow.x) + fabsf(ow.y)) + fabsf(ow.z)) + extent);
    const float dmax = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
    boxray_object(b, oo, od, mk3(W * nrm.x, W * nrm.y, W * nrm.z), mk3(nrm.x * dmax, nrm.y * dmax, nrm.z * dmax), no_cull);
    b.keep = (i3.y & sc.cull) != 0u ? 0xffu : 0u;
    return i4.z;
}

// model_matrix * (p, 1): ((m0 x + m1 y) + m2 z) + m3 per row — the bits of device_math.h mul_m4 with w = 1 (m3 * 1 is exact)
HR_DEV f3 instance_point(const InstanceIn& in, float x, float y, float z)
{
    return mk3(((in.m[0] * x + in.m[3] * y) + in.m[6] * z) + in.m[9], ((in.m[1] * x + in.m[4] * y) + in.m[7] * z) + in.m[10],
               ((in.m[2] * x + in.m[5] * y) + in.m[8] * z) + in.m[11]);
}

// the world-space vertices of a leaf triangle of the instance
HR_DEV void instance_tri(const InstanceIn& in, const TriRaw& q, f3& v0, f3& v1, f3& v2)
{
    v0 = instance_point(in, __uint_as_float(q.a.x), __uint_as_float(q.a.y), __uint_as_float(q.a.z));
    v1 = instance_point(in, __uint_as_float(q.b.x), __uint_as_float(q.b.y), __uint_as_float(q.b.z));
    v2 = instance_point(in, __uint_as_float(q.c.x), __uint_as_float(q.c.y), __uint_as_float(q.c.z));
}

struct Hit2
{
    float    t, u, v;
    int32_t  prim;   // global triangle index (instance order, then mesh order); -1 = miss.  ANY: 0 = occluded
    uint32_t inst;   // record (= top-level leaf) of the hit instance
    uint32_t local;  // mesh-local triangle index
    static HR_DEV Hit2 miss(float t_max) { return Hit2 { t_max, 0.0f, 0.0f, -1, 0u, 0u }; }
};

// ANY: any-hit (a pure function of ray and triangle set).  Otherwise closest hit: smallest t, ties to the smallest global triangle index.
// entry: the TOP-LEVEL node the walk starts from (0 = the root; HR_NO_ENTRY: nothing to walk, a miss).  entry_node_for_box (traverse.h) over a
// shared scene's `nodes` yields one: it descends through internal children only and stops at the first node with a leaf — an instance — among
// the overlapping children, so it never leaves the top level.  Any valid entry gives the root's answer.
// CUTOUT: traverse.h trace_any; the attribute index is the mesh's offset + the local triangle, the barycentrics are the world-space test's.
template <bool ANY, bool STATS = false, bool CUTOUT = false>
HR_DEV Hit2 trace2(const Scene2& sc, f3 o, f3 d, float t_min, float t_max, uint32_t* wave_stack, int lane, uint32_t* n_nodes = nullptr, uint32_t* n_tris = nullptr,
                   uint32_t entry = 0u, const CutoutView& cv = CutoutView())
{
    static_assert(!(STATS && CUTOUT), "no statistics build of the cutout walks");
    constexpr int ORDER = ANY ? HR_ANY_ORDER : HR_ORDER_NEAR;
    const RayPre rw = ray_prepare(o, d);   // world space: the top level's boxes and every triangle test
    BoxRay   br;
    boxray_world(br, rw);
    uint32_t  spill_array[HR_SPILL_ENTRIES];
    LaneStack st;
    st.init(wave_stack, lane, spill_array);
    uint32_t cur = (entry << 9) | 1u, ni;   // the entry node (the top level's root is node 0) = "child 0 of child_base entry"
    uint32_t pend = 0u, pend_base = 0u, slot = 0u;   // instances the last top-level node hit and the walk has not entered yet
    int      sp_base = 0;           // stack height at which the level being walked is exhausted
    bool     inside = false;
    InstanceIn in;
    Hit2 best = Hit2::miss(t_max);
    if (entry == HR_NO_ENTRY) return best;
    for (;;)
    {
        if ((cur & 0xffu) == 0u && st.sp == sp_base)
        {
            if (pend)
            {
                slot = pend_base + (uint32_t)__builtin_ctz(pend);
                pend &= pend - 1u;
                cur = (enter_instance(sc, slot, o, d, in, br) << 9) | 1u;
                inside = true;
            }
            else if (inside)
            {
                inside = false; sp_base = 0;   // back to the top level: its entries lie on the stack below
                boxray_world(br, rw);
                continue;
            }
            else
                break;
        }
        walk_next<ORDER != HR_ORDER_SLOTS>(cur, st, ni);
        const float    tfar = (ANY || best.prim < 0) ? t_max : best.t * 1.0000005f;
        const NodeHits h    = test_node2<ORDER>(load_node(sc.nodes, ni), br, t_min, tfar);
        if (STATS) (*n_nodes)++;
        uint32_t trimask = walk_expand(h, cur, st);
        if (!inside)
        {
            if (trimask)
            {
                // leaves of the top level are instances: park the top level's walk on the stack and enter them one after the other
                pend = trimask; pend_base = h.tri_base;
                if (cur & 0xffu) st.push(cur);
                cur = 0u; sp_base = st.sp;
            }
            continue;
        }
        while (trimask)
        {
            const uint32_t i = (uint32_t)__builtin_ctz(trimask);
            trimask &= trimask - 1u;
            const TriRaw q = load_tri_raw(sc.tris, h.tri_base + i);
            if (STATS) (*n_tris)++;
            f3 v0, v1, v2;
            instance_tri(in, q, v0, v1, v2);
            float t, u, v;
            if (ray_tri<!ANY || CUTOUT>(rw, v0, v1, v2, t_min, t_max, t, u, v) && (!CUTOUT || cutout_accept(cv, (size_t)in.mesh_tri_base + q.a.w, u, v)))
            {
                if (ANY) { best.prim = 0; best.inst = slot; best.local = q.a.w; return best; }
                const int32_t prim = (int32_t)(in.first_tri + q.a.w);
                if (best.prim < 0 || t < best.t || (t == best.t && prim < best.prim)) { best.t = t; best.u = u; best.v = v; best.prim = prim; best.inst = slot; best.local = q.a.w; }
            }
        }
    }
    return best;
}

// ---- wave-cooperative triangle tests on two levels (traverse.h trace_coop) --------------------------------------------------------------------
// A lane appends (owner lane, triangle reference, instance record) jobs to a ring in LDS and keeps walking; when the ring holds a job for every
// lane, each lane takes one: it fetches the owner's WORLD ray by __shfl as coop_flush does, loads the twelve matrix floats and first_tri of
// inst[slot], transforms the three vertices with instance_tri and runs trace2's ray_tri on trace2's operands — the decisions are bit-identical.
// Closest hit: 64-bit ds_min of ordered(t) << 32 | GLOBAL triangle (the reference's tie rule); the winner leaves u, v, the record and the
// mesh-local triangle beside it.  The far limit a lane culls nodes with lags by at most one flush.  Inactive lanes serve as job lanes.
struct CoopWave2
{
    uint2              jobs[HR_COOP_RING];   // x: triangle reference (< 2^31), y: owner lane << 26 | instance record (fewer than 2^23 of them)
    unsigned long long key[64];              // closest: ordered(t) << 32 | global prim, ~0 = miss;  any-hit: 0 = occluded
    float2             uv[64];
    uint2              where[64];            // closest: record, mesh-local triangle of the winner
};

template <bool ANY, bool CUTOUT = false>
HR_DEV void coop_flush2(CoopWave2& cw, const Scene2& sc, const RayPre& r, float t_min, float t_max, uint32_t rank, uint32_t head, uint32_t n, int lane,
                        const CutoutView& cv = CutoutView())
{
    const bool  mine  = rank < n;
    const uint2 job   = mine ? cw.jobs[(head + rank) & (HR_COOP_RING - 1)] : make_uint2(0u, (uint32_t)lane << 26);
    const int   owner = (int)(job.y >> 26);
    const uint32_t slot = job.y & ((1u << 26) - 1u);
    RayPre q;
    q.o.x = __shfl(r.o.x, owner); q.o.y = __shfl(r.o.y, owner); q.o.z = __shfl(r.o.z, owner);
    q.Sx  = __shfl(r.Sx, owner);  q.Sy  = __shfl(r.Sy, owner);  q.Sz  = __shfl(r.Sz, owner);
    const int kp = __shfl(r.kx | (r.ky << 2) | (r.kz << 4), owner);
    q.kx = kp & 3; q.ky = (kp >> 2) & 3; q.kz = kp >> 4;
    const float q_min = __shfl(t_min, owner), q_max = __shfl(t_max, owner);
    bool     hit = false;
    float    t = 0.0f, u = 0.0f, v = 0.0f;
    uint32_t prim = 0u, local = 0u;
    if (mine)
    {
        InstanceIn in;
        load_instance_in(sc.inst, slot, in);
        const TriRaw tr = load_tri_raw(sc.tris, job.x);
        f3 v0, v1, v2;
        instance_tri(in, tr, v0, v1, v2);
        hit   = ray_tri<!ANY || CUTOUT>(q, v0, v1, v2, q_min, q_max, t, u, v);
        local = tr.a.w;
        prim  = in.first_tri + local;
        if (CUTOUT) hit = hit && cutout_accept(cv, (size_t)in.mesh_tri_base + local, u, v);   // before key[owner] hears of the hit
    }
    if (ANY)
    {
        if (hit) cw.key[owner] = 0ull;
    }
    else
    {
        const unsigned long long k = ((unsigned long long)float_ordered(t) << 32) | prim;
        if (hit) atomicMin(&cw.key[owner], k);
        wave_fence();
        if (hit && cw.key[owner] == k) { cw.uv[owner] = make_float2(u, v); cw.where[owner] = make_uint2(slot, local); }
    }
    wave_fence();
}

// trace2's answer bit for bit (ANY: Hit2.prim = 0 if occluded, -1 if not; t, u, v, inst, local unset).  The caller keeps the wave converged
// around the call; lanes without a ray pass active = false.
template <bool ANY, bool CUTOUT = false>
HR_DEV Hit2 trace_coop2(bool active, const Scene2& sc, f3 o, f3 d, float t_min, float t_max, uint32_t* wave_stack, CoopWave2& cw, int lane, uint32_t entry = 0u,
                        const CutoutView& cv = CutoutView())
{
    constexpr int ORDER = ANY ? HR_ANY_ORDER : HR_ORDER_NEAR;
    const unsigned long long exec  = __ballot(1);
    const uint32_t           nproc = (uint32_t)__popcll(exec), rank = lanes_below(exec);
    const RayPre rw = ray_prepare(o, d);
    BoxRay   br;
    boxray_world(br, rw);
    uint32_t  spill_array[HR_SPILL_ENTRIES];
    LaneStack st;
    st.init(wave_stack, lane, spill_array);
    bool     alive = active && entry != HR_NO_ENTRY, inside = false;
    uint32_t cur   = alive ? ((entry << 9) | 1u) : 0u;
    uint32_t ipend = 0u, ipend_base = 0u, slot = 0u;   // instances of the last top-level node still to enter
    uint32_t tpend = 0u, tpend_base = 0u;              // leaf triangles of the last mesh node still to append
    int      sp_base = 0;
    uint32_t head = 0u, count = 0u;                    // wave-uniform
    float    tfar = t_max;
    InstanceIn in;
    cw.key[lane] = ~0ull;
    wave_fence();
    for (;;)
    {
        if (alive && tpend == 0u)
        {
            bool step = true;
            if ((cur & 0xffu) == 0u && st.sp == sp_base)
            {
                if (ipend)
                {
                    slot = ipend_base + (uint32_t)__builtin_ctz(ipend);
                    ipend &= ipend - 1u;
                    cur = (enter_instance(sc, slot, o, d, in, br) << 9) | 1u;
                    inside = true;
                }
                else if (inside)
                {
                    inside = false; sp_base = 0;
                    boxray_world(br, rw);
                    step = st.sp != 0;   // the parked top-level entries, if any
                    alive = step;
                }
                else { alive = false; step = false; }
            }
            if (step)
            {
                uint32_t ni;
                walk_next<ORDER != HR_ORDER_SLOTS>(cur, st, ni);
                const NodeHits h = test_node2<ORDER>(load_node(sc.nodes, ni), br, t_min, tfar);
                const uint32_t trimask = walk_expand(h, cur, st);
                if (inside) { tpend = trimask; tpend_base = h.tri_base; }
                else if (trimask)
                {
                    ipend = trimask; ipend_base = h.tri_base;
                    if (cur & 0xffu) st.push(cur);
                    cur = 0u; sp_base = st.sp;
                }
            }
        }
        uint32_t left = (uint32_t)__popc(tpend);
        uint32_t pos  = head + count;
#pragma unroll
        for (int k = 0; k < HR_COOP_PUSH; k++)
        {
            const bool               has = left > (uint32_t)k;
            const unsigned long long b   = __ballot(has);
            if (has)
            {
                const uint32_t i = (uint32_t)__builtin_ctz(tpend);
                tpend &= tpend - 1u;
                cw.jobs[(pos + lanes_below(b)) & (HR_COOP_RING - 1)] = make_uint2(tpend_base + i, ((uint32_t)lane << 26) | slot);
            }
            pos += (uint32_t)__popcll(b);
        }
        count = pos - head;
        const bool walking = __ballot(alive) != 0ull;
        bool       flushed = false;
        while (count >= nproc || (!walking && count > 0u))
        {
            const uint32_t n = count < nproc ? count : nproc;
            wave_fence();
            coop_flush2<ANY, CUTOUT>(cw, sc, rw, t_min, t_max, rank, head, n, lane, cv);
            head += n; count -= n;
            flushed = true;
        }
        if (flushed)
        {
            const unsigned long long k = cw.key[lane];
            if (ANY) { if (k == 0ull) { alive = false; tpend = 0u; } }
            else if (k != ~0ull) tfar = ordered_float((uint32_t)(k >> 32)) * 1.0000005f;
        }
        if (!walking && count == 0u) break;
    }
    Hit2 best = Hit2::miss(t_max);
    const unsigned long long k = cw.key[lane];
    if (ANY) { if (k == 0ull) best.prim = 0; }
    else if (k != ~0ull)
    {
        const float2 uv = cw.uv[lane];
        const uint2  w  = cw.where[lane];
        best.t = ordered_float((uint32_t)(k >> 32)); best.u = uv.x; best.v = uv.y; best.prim = (int32_t)(uint32_t)k; best.inst = w.x; best.local = w.y;
    }
    wave_fence();   // the next call re-initialises key[]
    return best;
}

template <bool CUTOUT = false>
HR_DEV bool   trace_any2(const Scene2& sc, f3 o, f3 d, float t_min, float t_max, uint32_t* wave_stack, int lane, uint32_t entry = 0u, const CutoutView& cv = CutoutView()) { return trace2<true, false, CUTOUT>(sc, o, d, t_min, t_max, wave_stack, lane, nullptr, nullptr, entry, cv).prim == 0; }
template <bool CUTOUT = false>
HR_DEV Hit2   trace_closest2(const Scene2& sc, f3 o, f3 d, float t_min, float t_max, uint32_t* wave_stack, int lane, const CutoutView& cv = CutoutView()) { return trace2<false, false, CUTOUT>(sc, o, d, t_min, t_max, wave_stack, lane, nullptr, nullptr, 0u, cv); }

} // namespace hr
