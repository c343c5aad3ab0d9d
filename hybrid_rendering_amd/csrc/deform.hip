// Deformable scenes: a flat scene whose vertices change every frame (cloth, a skinned character, foliage in wind, a morph target) while its
// topology — triangle count and order — stands.  hr_scene_create_deformable builds the 8-wide BVH once, on the host, with spatial splits OFF:
// every (finite) triangle then has exactly ONE reference and a leaf's box is the bounds of its triangles plus the builder's pad, so a refit needs
// no cells (instances.hip needs them because its trees are split).  What giving up the splits costs a trace is measured in docs/EXPERIMENTS.md.
//
// hr_scene_update_vertices (all on the caller's stream, no host synchronisation, no host mirror) is deform_refit.hip's scatter and refit of ONE
// mesh — the scene: root 0, the scene's `positions` / `tri_normals` as the scatter's rows, levels of up to 512 nodes in the one-workgroup launch
// (the launch shape of instances.hip), no bounds given and the root box it publishes ignored.  hr_scene_refit_cost is that mesh's cost.
// A refit never changes which triangles share a leaf, so a query's ANSWER is the one a fresh build over the same vertices gives (any-hit is a
// function of the triangle set, closest hit is the smallest t with ties to the smallest triangle index); only the boxes' quality decays.
// That holds for hostile vertices too (tests/test_gpu_deform_edges.py): a triangle with a NaN or infinite coordinate gets no box, as the builder
// gives it no reference — it is never hit, its leaf keeps the other triangles' bounds, a leaf or node with nothing finite in it is stored inverted
// and stays out of its parent's box (refit.h) — and comes back with its next finite vertices; and the leaf pad is the builder's rule applied to the
// CURRENT exact bounds of the finite triangles (instance_math.h leaf_pad, from k_deform_bounds on the same stream: no host synchronisation), so a
// scene created from a placeholder, inflated, collapsed or drifted away is padded for the size and place it has now.
// A triangle that was not finite when the scene was BUILT (created or rebuilt) has no reference to update: it stays out until the next host
// rebuild, or until a device re-deal hands it a slot that a triangle which is not finite NOW gives up (deform_redeal.hip).
// Two ways back from a decayed tree, neither called automatically: hr_scene_rebuild, the slow one (vertices read back, host SAH build, upload,
// new device arrays), and hr_scene_rebuild_device (deform_redeal.hip: kernels only — the tree's shape stands, its triangles are re-dealt among
// its leaves in Morton order and the refit runs; it does not reach a SAH build's quality).
#include "deform_refit.h"
#include "instance_math.h"
#include "scene_create.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

using namespace hr;

namespace {

constexpr int kNarrowLevel = 512;   // levels of at most this many nodes, from the root down to the first wider one, go to the one-workgroup launch

// ordered-integer image of a float: unsigned comparison == float comparison
__device__ uint32_t ordered_bits(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
float ordered_float(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// exact bounds of the finite triangles (the builder's rule, bvh_build.cpp): bits[0..2] min, bits[3..5] max, one atomic pair per axis per wave
__global__ __launch_bounds__(256) void k_deform_bounds(const float* positions, int n_tris, uint32_t* bits)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (t < n_tris)
    {
        const float* p = positions + (size_t)t * 9;
        float v[9];
        bool  finite = true;
        for (int k = 0; k < 9; k++) { v[k] = p[k]; finite = finite && fabsf(v[k]) < INFINITY; }
        if (finite)
            for (int k = 0; k < 9; k++) { lo[k % 3] = fminf(lo[k % 3], v[k]); hi[k % 3] = fmaxf(hi[k % 3], v[k]); }
    }
    for (int k = 0; k < 3; k++)
    {
        float l = lo[k], h = hi[k];
        for (int o = 32; o > 0; o >>= 1) { l = fminf(l, __shfl_xor(l, o)); h = fmaxf(h, __shfl_xor(h, o)); }
        if ((threadIdx.x & 63) == 0 && l <= h) { atomicMin(bits + k, ordered_bits(l)); atomicMax(bits + 3 + k, ordered_bits(h)); }
    }
}

void swap_buf(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }

hr_status not_deformable(const hr_scene* scene, const char* call)
{
    if (!scene) { set_last_error(std::string(call) + ": scene is NULL"); return HR_ERR_INVALID_ARG; }
    if (scene->n_instances > 0) { set_last_error(std::string(call) + ": an instanced scene cannot deform (hr_scene_update_instances moves its instances)"); return HR_ERR_INVALID_ARG; }
    if (!scene->deformable) { set_last_error(std::string(call) + ": not a deformable scene (hr_scene_create_deformable)"); return HR_ERR_INVALID_ARG; }
    return HR_OK;
}

hr_status rebuild_impl(hr_scene* s, hipStream_t st)
{
    HR_HIP(hipSetDevice(s->ctx->device));
    HR_HIP(hipStreamSynchronize(st));
    const int n = s->info.n_tris;
    std::vector<float> pos((size_t)n * 9);
    if (n > 0) HR_HIP(hipMemcpy(pos.data(), s->positions.p, pos.size() * 4, hipMemcpyDeviceToHost));
    BuiltBVH b;
    build_bvh8(pos.data(), n, b, false);
    if (b.nodes.size() >= (1u << 23)) { set_last_error("hr_scene_rebuild: more than 2^23 BVH nodes"); return HR_ERR_UNSUPPORTED; }
    if (b.max_depth >= kMaxTraversalDepth)
    {
        set_last_error("hr_scene_rebuild: BVH depth " + std::to_string(b.max_depth) + " exceeds the traversal stack (" + std::to_string(kMaxTraversalDepth) + ")");
        return HR_ERR_UNSUPPORTED;
    }
    // the new arrays stand complete before the scene lets go of the old ones
    DevBuf nodes, tris;
    hr_status e;
    if ((e = nodes.alloc(b.nodes.size() * sizeof(Node8))) != HR_OK) return e;
    if ((e = tris.alloc(b.tris.size() * sizeof(TriGPU))) != HR_OK) return e;
    HR_HIP(hipMemcpy(nodes.p, b.nodes.data(), b.nodes.size() * sizeof(Node8), hipMemcpyHostToDevice));
    if (!b.tris.empty()) HR_HIP(hipMemcpy(tris.p, b.tris.data(), b.tris.size() * sizeof(TriGPU), hipMemcpyHostToDevice));
    const hr_scene_info before = s->info;
    swap_buf(s->nodes, nodes); swap_buf(s->tris, tris);
    s->info.n_nodes    = (int32_t)b.nodes.size();
    s->info.max_depth  = b.max_depth;
    s->info.node_bytes = b.nodes.size() * sizeof(Node8);
    s->info.tri_bytes  = b.tris.size() * sizeof(TriGPU);
    s->info.box_pad    = b.pad;
    if ((e = deformable_scene_adopt(s, b)) != HR_OK)
    {
        swap_buf(s->nodes, nodes); swap_buf(s->tris, tris);   // the tree and the refit state of before stand
        s->info = before;
        return e;
    }
    for (int a = 0; a < 3; a++) { s->info.bounds_lo[a] = s->grid_lo[a] = b.lo[a]; s->info.bounds_hi[a] = s->grid_hi[a] = b.hi[a]; }
    s->bounds_stale = false;
    s->geometry_epoch++;
    return HR_OK;
}

} // namespace

// api.hip scene_create_impl / rebuild_impl: `s` holds the uploaded tree of `b` (built without spatial splits) and its info; sets up what a refit
// needs (deform_refit_adopt of one mesh, replacing what an earlier tree left) and the bounds read-back.  Synchronous, like creation.
hr_status hr::deformable_scene_adopt(hr_scene* s, const BuiltBVH& b)
{
    const DeformMesh m = { &b, 0u, 0u, 0u, s->info.n_tris, s->info.box_pad, true, kNarrowLevel };
    hr_status e;
    if ((e = s->bounds_bits.alloc(24)) != HR_OK) return e;
    if ((e = deform_refit_adopt(s, { m }, "deformable scene")) != HR_OK) return e;   // last: what fails before it leaves the scene's refit state alone
    s->deformable = true;
    return HR_OK;
}

// hr_scene_get_info of a deformable scene: the exact bounds of the last update, read back on demand (synchronises the device)
hr_status hr::deformable_scene_refresh_bounds(const hr_scene* scene)
{
    if (!scene->bounds_stale) return HR_OK;
    hr_scene* s = const_cast<hr_scene*>(scene);
    HR_HIP(hipSetDevice(s->ctx->device));
    HR_HIP(hipDeviceSynchronize());
    uint32_t bits[6] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u };
    HR_HIP(hipMemcpy(s->bounds_bits.p, bits, 24, hipMemcpyHostToDevice));
    const int n = s->info.n_tris;
    if (n > 0) hipLaunchKernelGGL(k_deform_bounds, dim3(cdiv(n, 256)), dim3(256), 0, nullptr, (const float*)s->positions.p, n, (uint32_t*)s->bounds_bits.p);
    HR_HIP(hipGetLastError());
    HR_HIP(hipMemcpy(bits, s->bounds_bits.p, 24, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++)
    {
        const bool any = bits[k] <= bits[3 + k] && bits[k] != 0xffffffffu;
        s->info.bounds_lo[k] = any ? ordered_float(bits[k]) : 0.0f;
        s->info.bounds_hi[k] = any ? ordered_float(bits[3 + k]) : 0.0f;
    }
    // the pad the last refit used: the builder's for these bounds (refit.h refit_pad)
    s->info.box_pad = imath::leaf_pad(s->info.bounds_lo, s->info.bounds_hi);
    s->bounds_stale = false;
    return HR_OK;
}

extern "C" {

hr_status hr_scene_create_deformable(hr_ctx* ctx, const hr_scene_desc* desc, hr_scene** out)
{
    return guarded("hr_scene_create_deformable", [&] { return scene_create_flat(ctx, desc, out, true); });
}

hr_status hr_scene_update_vertices(hr_scene* scene, const float* positions, const float* normals, int32_t first_tri, int32_t n_tris, void* stream)
{
    const hr_status nd = not_deformable(scene, "hr_scene_update_vertices");
    if (nd != HR_OK) return nd;
    if (!positions) { set_last_error("hr_scene_update_vertices: positions is NULL"); return HR_ERR_INVALID_ARG; }
    if (first_tri < 0 || n_tris < 0 || (int64_t)first_tri + n_tris > (int64_t)scene->info.n_tris)
    {
        set_last_error("hr_scene_update_vertices: triangles [" + std::to_string(first_tri) + ", " + std::to_string((int64_t)first_tri + n_tris) + ") outside the scene's " + std::to_string(scene->info.n_tris));
        return HR_ERR_INVALID_ARG;
    }
    if (normals && !scene->has_normals) { set_last_error("hr_scene_update_vertices: normals given for a scene created without normals"); return HR_ERR_INVALID_ARG; }
    if (n_tris == 0) return HR_OK;
    hipStream_t st = (hipStream_t)stream;
    HR_HIP(hipSetDevice(scene->ctx->device));
    const DeformScatterEntry entry = { positions, normals, 0u, first_tri, n_tris };
    deform_refit_scatter(scene, &entry, 1, (float*)scene->positions.p, normals ? (float*)scene->tri_normals.p : nullptr, st);
    const uint32_t mesh = 0u;
    const hr_status e = deform_refit_enqueue(scene, (Node8*)scene->nodes.p, &mesh, 1, nullptr, st);
    if (e != HR_OK) return e;
    scene->geometry_epoch++;
    scene->bounds_stale = true;
    scene->deform->cost_known[0] = 0;
    return HR_OK;
}

hr_status hr_scene_refit_cost(const hr_scene* scene, float* ratio)
{
    const hr_status nd = not_deformable(scene, "hr_scene_refit_cost");
    if (nd != HR_OK) return nd;
    if (!ratio) { set_last_error("hr_scene_refit_cost: ratio is NULL"); return HR_ERR_INVALID_ARG; }
    hr_scene* s = const_cast<hr_scene*>(scene);
    if (!s->deform->cost_known[0])
    {
        HR_HIP(hipSetDevice(s->ctx->device));
        HR_HIP(hipDeviceSynchronize());
    }
    return deform_refit_cost(s, 0u, ratio);
}

hr_status hr_scene_rebuild(hr_scene* scene, void* stream)
{
    const hr_status nd = not_deformable(scene, "hr_scene_rebuild");
    if (nd != HR_OK) return nd;
    try
    {
        return rebuild_impl(scene, (hipStream_t)stream);
    }
    catch (const std::bad_alloc&)
    {
        set_last_error("hr_scene_rebuild: host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
    catch (const std::exception& e)
    {
        set_last_error(std::string("hr_scene_rebuild: ") + e.what());
        return HR_ERR_UNSUPPORTED;
    }
}

} // extern "C"
