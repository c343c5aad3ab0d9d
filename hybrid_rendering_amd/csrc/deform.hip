// Deformable scenes: a flat scene whose vertices change every frame (cloth, a skinned character, foliage in wind, a morph target) while its
// topology — triangle count and order — stands.  hr_scene_create_deformable builds the 8-wide BVH once, on the host, with spatial splits OFF:
// every (finite) triangle then has exactly ONE reference and a leaf's box is the bounds of its triangles plus the builder's pad, so a refit needs
// no cells (instances.hip needs them because its trees are split).  What giving up the splits costs a trace is measured in docs/EXPERIMENTS.md.
//
// hr_scene_update_vertices (all on the caller's stream, no host synchronisation, no host mirror):
//   k_deform_scatter        one thread per updated triangle: the 36 vertex bytes of its reference (through the triangle -> reference map), its
//                           `positions` and, when given, its `tri_normals` (the hit shading and the G-buffer synthesiser read both)
//   k_deform_refit[_top]    refit.h refit_node<false>, one launch per WIDE tree level, deepest first, then one single-workgroup launch for the narrow
//                           levels near the root (a barrier between levels) — the launch shape of instances.hip.  Launch boundaries are the only
//                           ordering between levels: the per-XCD L2s are not coherent with each other (see the header of instances.hip).
//                           Every node is refitted, whatever the updated range: a parent's box depends on all its leaves.
// The refit cost (hr_scene_refit_cost: sum of the nodes' half areas now / when built — the measure the instanced scenes' top-level re-build
// trigger uses, top_area_at_build) rides in the refit: every workgroup reduces its nodes' areas (double, a fixed butterfly) and stores ONE partial
// sum in its own slot with a plain vector store; the host adds the slots in index order when the ratio is asked for.  No atomic: a sum in arrival
// order would not reproduce, and "the same vertices give exactly 1.0" is a test of the refit's encoding.
// A refit never changes which triangles share a leaf, so a query's ANSWER is the one a fresh build over the same vertices gives (any-hit is a
// function of the triangle set, closest hit is the smallest t with ties to the smallest triangle index); only the boxes' quality decays.
// hr_scene_rebuild is the slow way back: vertices read back, host build, upload.  Nothing calls it automatically.
#include "hr_internal.h"
#include "refit.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

using namespace hr;

namespace {

__global__ __launch_bounds__(64) void k_deform_refit(RefitArgs a, double* partial)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    double area = 0.0;
    if (i < a.count) area = refit_node<false>(a, a.list[i]);
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if (threadIdx.x == 0) partial[blockIdx.x] = area;
}

// the narrow levels near the root in ONE workgroup (instances.hip k_instances_refit_top)
struct RefitTopArgs { RefitArgs r; const uint32_t* lists; double* partial; int offs[kMaxTraversalDepth + 2]; int d_top; };
__global__ __launch_bounds__(256) void k_deform_refit_top(RefitTopArgs t)
{
    __shared__ double s_sum[4];
    double area = 0.0;
    for (int d = t.d_top; d >= 0; d--)
    {
        for (int i = t.offs[d] + (int)threadIdx.x; i < t.offs[d + 1]; i += 256) area += refit_node<false>(t.r, t.lists[i]);
        __threadfence_block();
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = area;
    __syncthreads();
    if (threadIdx.x == 0) t.partial[0] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

struct ScatterArgs
{
    TriGPU*        tris;
    const int32_t* tri_ref;      // per original triangle: index of its reference, -1: none (not finite when the tree was built)
    float*         positions;    // scene, by original triangle
    float*         normals;      // scene, or null
    const float*   src_positions;
    const float*   src_normals;  // or null
    int            first, count;
};

__global__ __launch_bounds__(256) void k_deform_scatter(ScatterArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.count) return;
    const size_t g = (size_t)a.first + t;
    const float* p = a.src_positions + (size_t)t * 9;
    float v[9];
    for (int k = 0; k < 9; k++) v[k] = p[k];
    float* w = a.positions + g * 9;
    for (int k = 0; k < 9; k++) w[k] = v[k];
    const int32_t r = a.tri_ref[g];
    if (r >= 0)
    {
        TriGPU& d = a.tris[r];   // prim and the padding words stand
        d.v0[0] = v[0]; d.v0[1] = v[1]; d.v0[2] = v[2];
        d.v1[0] = v[3]; d.v1[1] = v[4]; d.v1[2] = v[5];
        d.v2[0] = v[6]; d.v2[1] = v[7]; d.v2[2] = v[8];
    }
    if (a.src_normals)
    {
        const float* n = a.src_normals + (size_t)t * 9;
        float*       o = a.normals + g * 9;
        for (int k = 0; k < 9; k++) o[k] = n[k];
    }
}

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

// the refit of every level of `s` into `nodes` (the scene's own array, or a scratch copy when only boxes and cost are wanted), on `st`
hr_status enqueue_refit(hr_scene* s, Node8* nodes, hipStream_t st)
{
    RefitArgs r;
    r.nodes = nodes; r.tris = (const TriGPU*)s->tris.p; r.node_box = (float*)s->node_box.p; r.pad = s->info.box_pad;
    r.cells = nullptr; r.node_inst = nullptr; r.inst = nullptr; r.dirty = nullptr; r.list = nullptr; r.count = 0;
    double* partial = (double*)s->cost_partials.p;
    const int n_levels = (int)s->level_offsets.size() - 1;
    int d_top = -1;
    while (d_top + 1 < n_levels && d_top + 1 <= kMaxTraversalDepth && s->level_offsets[(size_t)d_top + 2] - s->level_offsets[(size_t)d_top + 1] <= 512) d_top++;
    int slot = 1;   // slot 0: the single-workgroup launch
    for (int d = n_levels - 1; d > d_top; d--)
    {
        r.list = (const uint32_t*)s->level_nodes.p + s->level_offsets[(size_t)d];
        r.count = s->level_offsets[(size_t)d + 1] - s->level_offsets[(size_t)d];
        if (r.count <= 0) continue;
        const int groups = cdiv(r.count, 64);
        if (slot + groups > s->n_cost_partials) { set_last_error("deformable scene: refit cost slots exhausted"); return HR_ERR_HIP; }
        hipLaunchKernelGGL(k_deform_refit, dim3(groups), dim3(64), 0, st, r, partial + slot);
        slot += groups;
    }
    RefitTopArgs t;
    t.r = r; t.lists = (const uint32_t*)s->level_nodes.p; t.partial = partial; t.d_top = d_top;
    for (int d = 0; d < kMaxTraversalDepth + 2; d++) t.offs[d] = 0;
    for (int d = 0; d <= d_top + 1; d++) t.offs[d] = s->level_offsets[(size_t)d];
    hipLaunchKernelGGL(k_deform_refit_top, dim3(1), dim3(256), 0, st, t);   // also with d_top = -1: it clears slot 0
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status read_cost(hr_scene* s, double* sum)
{
    std::vector<double> part((size_t)s->n_cost_partials);
    HR_HIP(hipMemcpy(part.data(), s->cost_partials.p, part.size() * 8, hipMemcpyDeviceToHost));
    double a = 0.0;
    for (double v : part) a += v;
    *sum = a;
    return HR_OK;
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
    swap_buf(s->nodes, nodes); swap_buf(s->tris, tris);
    s->info.n_nodes    = (int32_t)b.nodes.size();
    s->info.max_depth  = b.max_depth;
    s->info.node_bytes = b.nodes.size() * sizeof(Node8);
    s->info.tri_bytes  = b.tris.size() * sizeof(TriGPU);
    s->info.box_pad    = b.pad;
    for (int a = 0; a < 3; a++) { s->info.bounds_lo[a] = s->grid_lo[a] = b.lo[a]; s->info.bounds_hi[a] = s->grid_hi[a] = b.hi[a]; }
    s->bounds_stale = false;
    if ((e = deformable_scene_adopt(s, b)) != HR_OK) return e;
    s->geometry_epoch++;
    return HR_OK;
}

} // namespace

// api.hip scene_create_impl / rebuild_impl: `s` holds the uploaded tree of `b` (built without spatial splits) and its info; sets up what a refit
// needs — the level lists, the triangle -> reference map, node_box (by one refit into a scratch copy of the nodes: the scene's own stay as built)
// and the cost of the tree as built.  Synchronous, like creation.
hr_status hr::deformable_scene_adopt(hr_scene* s, const BuiltBVH& b)
{
    const size_t n_nodes = b.nodes.size();
    const int    n_tris = s->info.n_tris;
    std::vector<int> depth(n_nodes, 0);   // children follow their parent in the builder's breadth-first order
    int max_depth = 0;
    for (size_t j = 0; j < n_nodes; j++)
        for (int c = 0; c < (b.nodes[j].counts & 15); c++) { depth[(size_t)b.nodes[j].child_base + c] = depth[j] + 1; max_depth = std::max(max_depth, depth[j] + 1); }
    s->level_offsets.assign((size_t)max_depth + 2, 0);
    for (size_t j = 0; j < n_nodes; j++) s->level_offsets[(size_t)depth[j] + 1]++;
    for (size_t d = 0; d + 1 < s->level_offsets.size(); d++) s->level_offsets[d + 1] += s->level_offsets[d];
    std::vector<uint32_t> level_nodes(n_nodes);
    {
        std::vector<int32_t> cur(s->level_offsets.begin(), s->level_offsets.end() - 1);
        for (size_t j = 0; j < n_nodes; j++) level_nodes[(size_t)cur[(size_t)depth[j]]++] = (uint32_t)j;
    }
    std::vector<int32_t> tri_ref((size_t)n_tris, -1);
    for (size_t r = 0; r < b.tris.size(); r++)
    {
        const uint32_t prim = b.tris[r].prim;
        if (prim >= (uint32_t)n_tris || tri_ref[prim] >= 0) { set_last_error("deformable scene: a triangle with more than one reference in a tree built without spatial splits"); return HR_ERR_UNSUPPORTED; }
        tri_ref[prim] = (int32_t)r;
    }
    int partials = 1;
    for (size_t d = 0; d + 1 < s->level_offsets.size(); d++) partials += cdiv(s->level_offsets[d + 1] - s->level_offsets[d], 64);
    hr_status e;
    if ((e = s->level_nodes.alloc(n_nodes * 4)) != HR_OK) return e;
    if ((e = s->tri_ref.alloc((size_t)n_tris * 4)) != HR_OK) return e;
    if ((e = s->node_box.alloc(n_nodes * 32)) != HR_OK) return e;
    if ((e = s->cost_partials.alloc((size_t)partials * 8)) != HR_OK) return e;   // zeroed: slots a launch shape leaves unused add nothing
    if ((e = s->bounds_bits.alloc(24)) != HR_OK) return e;
    s->n_cost_partials = partials;
    HR_HIP(hipMemcpy(s->level_nodes.p, level_nodes.data(), n_nodes * 4, hipMemcpyHostToDevice));
    if (n_tris > 0) HR_HIP(hipMemcpy(s->tri_ref.p, tri_ref.data(), (size_t)n_tris * 4, hipMemcpyHostToDevice));
    DevBuf scratch;
    if ((e = scratch.alloc(n_nodes * sizeof(Node8))) != HR_OK) return e;
    HR_HIP(hipMemcpy(scratch.p, s->nodes.p, n_nodes * sizeof(Node8), hipMemcpyDeviceToDevice));
    if ((e = enqueue_refit(s, (Node8*)scratch.p, nullptr)) != HR_OK) return e;
    HR_HIP(hipStreamSynchronize(nullptr));
    if ((e = read_cost(s, &s->cost_at_build)) != HR_OK) return e;
    s->cost_ratio = 1.0;
    s->cost_stale = false;
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
    s->bounds_stale = false;
    return HR_OK;
}

extern "C" {

hr_status hr_scene_create_deformable(hr_ctx* ctx, const hr_scene_desc* desc, hr_scene** out)
{
    try
    {
        return scene_create_flat(ctx, desc, out, true);
    }
    catch (const std::bad_alloc&)
    {
        set_last_error("hr_scene_create_deformable: host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
    catch (const std::exception& e)
    {
        set_last_error(std::string("hr_scene_create_deformable: ") + e.what());
        return HR_ERR_UNSUPPORTED;
    }
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
    ScatterArgs a;
    a.tris = (TriGPU*)scene->tris.p; a.tri_ref = (const int32_t*)scene->tri_ref.p; a.positions = (float*)scene->positions.p;
    a.normals = normals ? (float*)scene->tri_normals.p : nullptr; a.src_positions = positions; a.src_normals = normals;
    a.first = first_tri; a.count = n_tris;
    hipLaunchKernelGGL(k_deform_scatter, dim3(cdiv(n_tris, 256)), dim3(256), 0, st, a);
    const hr_status e = enqueue_refit(scene, (Node8*)scene->nodes.p, st);
    if (e != HR_OK) return e;
    scene->geometry_epoch++;
    scene->bounds_stale = true;
    scene->cost_stale = true;
    return HR_OK;
}

hr_status hr_scene_refit_cost(const hr_scene* scene, float* ratio)
{
    const hr_status nd = not_deformable(scene, "hr_scene_refit_cost");
    if (nd != HR_OK) return nd;
    if (!ratio) { set_last_error("hr_scene_refit_cost: ratio is NULL"); return HR_ERR_INVALID_ARG; }
    hr_scene* s = const_cast<hr_scene*>(scene);
    if (s->cost_stale)
    {
        HR_HIP(hipSetDevice(s->ctx->device));
        HR_HIP(hipDeviceSynchronize());
        double now = 0.0;
        const hr_status e = read_cost(s, &now);
        if (e != HR_OK) return e;
        s->cost_ratio = s->cost_at_build > 0.0 ? now / s->cost_at_build : 1.0;
        s->cost_stale = false;
    }
    *ratio = (float)s->cost_ratio;
    return HR_OK;
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
