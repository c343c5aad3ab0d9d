// hr_scene_rebuild_device / hr_scene_rebuild_meshes_device: the way back for a deformable mesh whose refitted tree has decayed, kernels only on the
// caller's stream, nothing read back.  Not a BVH builder: the node topology stays exactly as the host built it — child_base, tri_base, every meta
// byte, the level lists, the partial slots — and what the device decides is WHICH triangle stands in which reference slot: the mesh's triangles
// sorted by the 30-bit Morton code of their box's centre inside the exact bounds of the mesh's finite references (instance_math.h sort_key over
// the triangle's mesh-local index: unique, so the order is a function of the vertices and those bounds alone), dealt in that order to the
// slots in depth-first order of the standing tree (deform_leaf_order: the builder's reference array is not subtree-contiguous), then the standing
// refit (deform_refit.hip).  Answers do not depend on the tree (any-hit is a function of the triangle set, closest hit the smallest t with ties
// to the smallest original index: traverse.h), so correctness never depends on this file's order — only on every slot holding a whole triangle
// and tri_ref naming it.  The design of instances_shared_rebuild.hip, one level down; the sorts are the same (device_sort.h).
//
// One engine for the flat deformable scenes (deform.hip: one mesh, the scene's `positions` rows) and the flagged meshes of a shared instanced
// scene (instances_shared_deform.hip: `mesh_positions`).  Per call, for meshes ms[0 .. n):
//   k_deform_bounds      (deform_refit.hip, one launch for all meshes) the exact bounds of each mesh's finite references into its bounds_bits words
//   per mesh, one after the other (they share the scratch buffers):
//     sort               n_tris <= kSortSmall: k_redeal_sort_small, keys made and sorted in ONE workgroup's LDS; else k_redeal_keys and the radix
//                        passes.  A triangle with a NaN or infinite coordinate gets the code 1 << 30, above every 30-bit code: it sorts last.
//                        With no finite reference the bounds are the builder's zero box: every finite triangle then has code 0.
//     k_redeal_gather    rank r < n_refs: the whole 48-byte record of the triangle of rank r into scratch — vertices from the positions row, prim and
//                        both padding words from the reference it has now (nothing keeps anything in them: the cutout table is keyed on prim,
//                        cutout.hip), or prim = the triangle and zeros when it has none
//     k_redeal_commit    scratch -> `tris` (the passes hold that pointer) at slot_of_rank[r]; tri_ref of every triangle: its slot, or -1 for rank
//                        >= n_refs — today's rule "no reference until the next host build", now applied to the triangles that sort last, the
//                        non-finite ones first of all; a triangle that was not finite when the tree was built gains a slot when one that is
//                        not finite now gives one up.  Its first lane puts the mesh's bounds_bits words back to idle for the refit.
//   deform_refit_enqueue over all n meshes.  cost_at_build stays the host build's: the cost ratio after a re-deal compares the re-dealt tree
//   with the SAH tree as built.
// Launch boundaries are the only ordering between these steps: the per-XCD L2s are not coherent with each other (instances.hip).
//
// Known limit: a triangle much larger than its Morton cell (a floor under furniture) lands in a small leaf by its centre and widens every
// ancestor; a SAH build would have isolated it near the root (docs/EXPERIMENTS.md "Device re-deal of a deformable mesh").
#include "deform_refit.h"
#include "device_sort.h"
#include "refit.h"
#include <algorithm>
#include <cstring>

using namespace hr;

namespace {

constexpr uint32_t kNonFiniteCode = 1u << 30;

struct RedealArgs
{
    TriGPU*         tris;
    TriGPU*         scratch;
    const float*    positions;      // the attribute rows of all meshes
    int32_t*        tri_ref;
    const int32_t*  slot_of_rank;   // at ref_base: the mesh's slots, global
    const uint32_t* order;          // rank -> mesh-local triangle
    uint32_t*       bits;           // the mesh's six words of bounds_bits
    uint32_t        tri_base, ref_base;
    int32_t         n_tris, n_refs;
};

// code of mesh-local triangle t: the Morton code of its box inside the bounds `bits` hold, or kNonFiniteCode
__device__ inline uint32_t tri_code(const float* positions, uint32_t tri_base, int t, const float* bounds)
{
    const float* p = positions + ((size_t)tri_base + (size_t)t) * 9;
    float v[9];
    bool  fin = true;
    for (int k = 0; k < 9; k++) { v[k] = p[k]; fin = fin && imath::finite_f(v[k]); }
    if (!fin) return kNonFiniteCode;
    float box[6];
    for (int k = 0; k < 3; k++)
    {
        box[k]     = imath::fmin_(v[k], imath::fmin_(v[3 + k], v[6 + k]));
        box[3 + k] = imath::fmax_(v[k], imath::fmax_(v[3 + k], v[6 + k]));
    }
    return imath::morton_code(box, bounds);
}
// the bounds k_deform_bounds reduced (wave-uniform: six scalar loads); no finite reference: the builder's zero box (refit.h refit_pad)
__device__ inline void bounds_of_bits(const uint32_t* bits, float* bounds)
{
    const bool any = bits[0] <= bits[3];
    for (int k = 0; k < 6; k++) bounds[k] = any ? ordered_float_dev(bits[k]) : 0.0f;
}

// blockDim.x == kSortLanes; n2: a power of two, n <= n2 <= kSortSmall
__global__ void __launch_bounds__(kSortLanes) k_redeal_sort_small(const float* positions, const uint32_t* bits, uint32_t tri_base, uint32_t* order, int n, int n2)
{
    __shared__ unsigned long long key[kSortSmall];
    const int t = (int)threadIdx.x;
    float bounds[6];
    bounds_of_bits(bits, bounds);
    for (int e = t; e < n2; e += kSortLanes)
        key[e] = e < n ? (((unsigned long long)tri_code(positions, tri_base, e, bounds) << 32) | (unsigned long long)e) : ~0ull;   // above every key
    __syncthreads();
    bitonic_sort_lds(key, n2, t);
    for (int e = t; e < n; e += kSortLanes) order[e] = (uint32_t)(key[e] & 0xffffffffull);
}

__global__ void __launch_bounds__(256) k_redeal_keys(const float* positions, const uint32_t* bits, uint32_t tri_base, uint32_t* codes, uint32_t* idx, int n)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    float bounds[6];
    bounds_of_bits(bits, bounds);
    codes[i] = tri_code(positions, tri_base, i, bounds);
    idx[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_redeal_gather(RedealArgs a)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= a.n_refs) return;
    const uint32_t tri = a.order[r];
    if (tri >= (uint32_t)a.n_tris) return;   // (never, while `order` is this call's: the guards keep a stale one inside the arrays)
    const size_t g = (size_t)a.tri_base + tri;
    const float* p = a.positions + g * 9;
    uint4 q0, q1, q2;
    q0.x = __float_as_uint(p[0]); q0.y = __float_as_uint(p[1]); q0.z = __float_as_uint(p[2]);
    q1.x = __float_as_uint(p[3]); q1.y = __float_as_uint(p[4]); q1.z = __float_as_uint(p[5]);
    q2.x = __float_as_uint(p[6]); q2.y = __float_as_uint(p[7]); q2.z = __float_as_uint(p[8]);
    q0.w = tri; q1.w = 0u; q2.w = 0u;
    const int32_t old = a.tri_ref[g];
    if (old >= (int32_t)a.ref_base && old - (int32_t)a.ref_base < a.n_refs)
    {
        const TriGPU& o = a.tris[old];
        q0.w = o.prim; q1.w = o.pad1; q2.w = o.pad2;
    }
    uint4* d = reinterpret_cast<uint4*>(a.scratch + r);
    d[0] = q0; d[1] = q1; d[2] = q2;
}

__global__ void __launch_bounds__(256) k_redeal_commit(RedealArgs a)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r == 0)
        for (int k = 0; k < 3; k++) { a.bits[k] = 0xffffffffu; a.bits[3 + k] = 0u; }   // their readers ran launches ago; the refit behind this reduces into them afresh
    if (r >= a.n_tris) return;
    const uint32_t tri = a.order[r];
    if (tri >= (uint32_t)a.n_tris) return;
    int32_t slot = -1;
    if (r < a.n_refs)
    {
        slot = a.slot_of_rank[(size_t)a.ref_base + r];
        if (slot < (int32_t)a.ref_base || slot - (int32_t)a.ref_base >= a.n_refs) return;
        const uint4* q = reinterpret_cast<const uint4*>(a.scratch + r);
        uint4*       d = reinterpret_cast<uint4*>(a.tris + slot);
        const uint4  q0 = q[0], q1 = q[1], q2 = q[2];
        d[0] = q0; d[1] = q1; d[2] = q2;
    }
    a.tri_ref[(size_t)a.tri_base + tri] = slot;
}

void swap_buf(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }

// the scratch buffers and the table's device copy: everything stands before the scene takes any of it
hr_status ensure_buffers(DeformRefit& sd)
{
    if (sd.redeal_ready) return HR_OK;
    size_t max_tris = 0, max_refs = 0;
    for (size_t m = 0; m < sd.flag.size(); m++)
        if (sd.flag[m]) { max_tris = std::max(max_tris, (size_t)sd.n_tris[m]); max_refs = std::max(max_refs, (size_t)sd.n_refs[m]); }
    DevBuf table, codes[2], idx[2], hist, tris;
    hr_status e;
    if ((e = table.alloc(sd.slot_of_rank_host.size() * 4)) != HR_OK) return e;
    for (int k = 0; k < 2; k++)
    {
        if ((e = codes[k].alloc(max_tris * 4)) != HR_OK) return e;
        if ((e = idx[k].alloc(max_tris * 4)) != HR_OK) return e;
    }
    if ((e = hist.alloc(radix_hist_bytes(max_tris))) != HR_OK) return e;
    if ((e = tris.alloc(max_refs * sizeof(TriGPU))) != HR_OK) return e;
    if (!sd.slot_of_rank_host.empty()) HR_HIP(hipMemcpy(table.p, sd.slot_of_rank_host.data(), sd.slot_of_rank_host.size() * 4, hipMemcpyHostToDevice));
    swap_buf(sd.rd_slot_of_rank, table); swap_buf(sd.rd_hist, hist); swap_buf(sd.rd_tris, tris);
    for (int k = 0; k < 2; k++) { swap_buf(sd.rd_codes[k], codes[k]); swap_buf(sd.rd_idx[k], idx[k]); }
    sd.redeal_ready = true;
    return HR_OK;
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

} // namespace

bool hr::deform_leaf_order(const Node8* nodes, int32_t n_nodes, uint32_t root, int32_t* slot_of_rank, int32_t capacity, int32_t* n)
{
    if (n_nodes <= 0 || root >= (uint32_t)n_nodes) return false;
    std::vector<int64_t> out;
    // an explicit stack of (node, next slot): a node's internal slots come first (bvh.h), so its subtrees precede its own leaves
    std::vector<std::pair<uint32_t, int>> stack;
    stack.push_back({ root, 0 });
    int64_t visits = 1, first = INT64_MAX;
    while (!stack.empty())
    {
        const uint32_t ni = stack.back().first;
        const int      c  = stack.back().second;
        const Node8&   nd = nodes[ni];
        const int n_internal = nd.counts & 15, n_children = nd.counts >> 4;
        if (c >= n_children || c >= 8) { stack.pop_back(); continue; }
        stack.back().second = c + 1;
        if (c < n_internal)
        {
            const uint64_t child = (uint64_t)nd.child_base + (uint64_t)c;
            if (child >= (uint64_t)n_nodes || ++visits > (int64_t)n_nodes) return false;
            stack.push_back({ (uint32_t)child, 0 });
        }
        else
        {
            const uint32_t m = nd.meta[c], cnt = m >> 5, off = m & 31u;
            for (uint32_t t = 0; t < cnt; t++)
            {
                const int64_t ref = (int64_t)nd.tri_base + off + t;
                if ((int64_t)out.size() >= (int64_t)capacity) return false;
                out.push_back(ref);
                first = std::min(first, ref);
            }
        }
    }
    for (size_t r = 0; r < out.size(); r++) slot_of_rank[r] = (int32_t)(out[r] - first);
    if (n) *n = (int32_t)out.size();
    return true;
}

hr_status hr::deform_redeal_enqueue(hr_scene* s, const uint32_t* ms, int n, hipStream_t st)
{
    static const char* call = "device re-deal";
    DeformRefit& sd = *s->deform;
    for (int j = 0; j < n; j++)
        if (!sd.redeal_ok[ms[j]]) { set_last_error(std::string(call) + ": the leaves of mesh " + std::to_string(ms[j]) + "'s tree do not name each of its references once"); return HR_ERR_UNSUPPORTED; }
    if (!sd.redeal_ready && stream_is_capturing(st)) return bad(call, "the first device re-deal of a scene allocates: not possible while the stream is capturing");
    hr_status e;
    if ((e = ensure_buffers(sd)) != HR_OK) return e;
    const float* positions = (const float*)(s->shared ? s->mesh_positions.p : s->positions.p);
    int64_t launched = 0;
    bool any_refs = false;
    for (int j = 0; j < n; j++) any_refs = any_refs || sd.n_refs[ms[j]] > 0;
    deform_refit_bounds_enqueue(s, ms, n, st);
    HR_HIP(hipGetLastError());
    if (any_refs) launched++;
    uint32_t* const codes[2] = { (uint32_t*)sd.rd_codes[0].p, (uint32_t*)sd.rd_codes[1].p };
    uint32_t* const idx[2]   = { (uint32_t*)sd.rd_idx[0].p, (uint32_t*)sd.rd_idx[1].p };
    for (int j = 0; j < n; j++)
    {
        const uint32_t m = ms[j];
        const int nt = sd.n_tris[m];
        if (nt <= 0) continue;
        uint32_t* bits = (uint32_t*)sd.bounds_bits.p + (size_t)m * 6;
        if (nt <= kSortSmall)
        {
            int n2 = 64;
            while (n2 < nt) n2 *= 2;
            hipLaunchKernelGGL(k_redeal_sort_small, dim3(1), dim3(kSortLanes), 0, st, positions, (const uint32_t*)bits, sd.tri_base[m], idx[0], nt, n2);
            HR_HIP(hipGetLastError());
            launched++;
        }
        else
        {
            hipLaunchKernelGGL(k_redeal_keys, dim3(cdiv(nt, 256)), dim3(256), 0, st, positions, (const uint32_t*)bits, sd.tri_base[m], codes[0], idx[0], nt);
            HR_HIP(hipGetLastError());
            launched++;
            if ((e = radix_sort_enqueue(codes, idx, (uint32_t*)sd.rd_hist.p, nullptr, nt, 0, st, &launched)) != HR_OK) return e;   // the order ends in idx[0]
        }
        RedealArgs a;
        a.tris = (TriGPU*)s->tris.p; a.scratch = (TriGPU*)sd.rd_tris.p; a.positions = positions; a.tri_ref = (int32_t*)sd.tri_ref.p;
        a.slot_of_rank = (const int32_t*)sd.rd_slot_of_rank.p; a.order = idx[0]; a.bits = bits;
        a.tri_base = sd.tri_base[m]; a.ref_base = sd.ref_base[m]; a.n_tris = nt; a.n_refs = sd.n_refs[m];
        if (a.n_refs > 0)
        {
            hipLaunchKernelGGL(k_redeal_gather, dim3(cdiv(a.n_refs, 256)), dim3(256), 0, st, a);
            HR_HIP(hipGetLastError());
            launched++;
        }
        hipLaunchKernelGGL(k_redeal_commit, dim3(cdiv(nt, 256)), dim3(256), 0, st, a);
        HR_HIP(hipGetLastError());
        launched++;
    }
    // the refit: for a shared scene against the bounds the mesh's instances stand on (the vertices have not changed, so what the last update's
    // check said of them stands)
    std::vector<const float*> bs((size_t)n, nullptr);
    if (s->shared)
        for (int j = 0; j < n; j++) bs[(size_t)j] = &s->mesh_bounds[(size_t)ms[j] * 6];
    // its launches count as the re-deal's: level_launches / top_launches stay "what the updates enqueued" (hr_scene_update_meshes_stats)
    const int64_t level_before = sd.level_launches, top_before = sd.top_launches;
    e = deform_refit_enqueue(s, (Node8*)s->nodes.p, ms, n, bs.data(), st);
    launched += (sd.level_launches - level_before) + (sd.top_launches - top_before) + (any_refs ? 1 : 0);
    sd.level_launches = level_before; sd.top_launches = top_before;
    if (e != HR_OK) { s->redeal_launches += launched; return e; }
    for (int j = 0; j < n; j++) sd.cost_known[ms[j]] = 0;
    s->redeals += n;
    s->redeal_launches += launched;
    return HR_OK;
}

extern "C" {

hr_status hr_deform_leaf_order(const void* nodes, int32_t n_nodes, uint32_t root, int32_t* slot_of_rank, int32_t capacity, int32_t* n)
{
    static const char* call = "hr_deform_leaf_order";
    try
    {
        if (!nodes || n_nodes < 1 || capacity < 0 || (capacity > 0 && !slot_of_rank)) return bad(call, "NULL argument, n_nodes < 1 or capacity < 0");
        std::vector<int32_t> out((size_t)capacity);
        int32_t count = 0;
        if (!deform_leaf_order((const Node8*)nodes, n_nodes, root, out.data(), capacity, &count))
            return bad(call, "capacity is below the tree's reference count, or the nodes are not a tree inside the array");
        if (count > 0) std::memcpy(slot_of_rank, out.data(), (size_t)count * 4);
        if (n) *n = count;
        return HR_OK;
    }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

hr_status hr_scene_rebuild_device(hr_scene* scene, void* stream)
{
    static const char* call = "hr_scene_rebuild_device";
    try
    {
        if (!scene) return bad(call, "scene is NULL");
        if (scene->n_instances > 0) return bad(call, "an instanced scene (hr_scene_rebuild_meshes_device re-deals the flagged meshes of a shared one)");
        if (!scene->deformable || !scene->deform) return bad(call, "not a deformable scene (hr_scene_create_deformable)");
        HR_HIP(hipSetDevice(scene->ctx->device));
        const uint32_t mesh = 0u;
        scene->geometry_epoch++;       // before the launches, so that it has moved also when an error leaves some of them in the stream
        scene->bounds_stale = true;
        return deform_redeal_enqueue(scene, &mesh, 1, (hipStream_t)stream);
    }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

hr_status hr_scene_rebuild_meshes_device(hr_scene* scene, const uint32_t* mesh_idx, int32_t n, void* stream)
{
    static const char* call = "hr_scene_rebuild_meshes_device";
    try
    {
        if (!scene) return bad(call, "scene is NULL");
        if (!scene->shared || !scene->deform) return bad(call, "not a scene from hr_scene_create_instanced_shared_deformable");
        if (n < 0 || (n > 0 && !mesh_idx)) return bad(call, "mesh_idx is NULL or n < 0");
        const DeformRefit& sd = *scene->deform;
        // everything is checked before anything is enqueued
        std::vector<uint8_t> named(sd.flag.size(), 0);
        for (int32_t i = 0; i < n; i++)
        {
            const uint32_t m = mesh_idx[i];
            const std::string where = "mesh_idx[" + std::to_string(i) + "]: ";
            if (m >= (uint32_t)sd.flag.size()) return bad(call, where + std::to_string(m) + " >= n_meshes " + std::to_string(sd.flag.size()));
            if (!sd.flag[m]) return bad(call, where + "mesh " + std::to_string(m) + " was not flagged deformable when the scene was created");
            if (named[m]) return bad(call, where + "mesh " + std::to_string(m) + " is named twice");
            named[m] = 1;
        }
        if (n == 0) return HR_OK;
        HR_HIP(hipSetDevice(scene->ctx->device));
        scene->geometry_epoch++;       // before the launches: an error in a later chunk of 64 leaves the earlier chunks' trees re-dealt
        for (int32_t at = 0; at < n; at += kMaxUpdatesPerLaunch)
        {
            const hr_status e = deform_redeal_enqueue(scene, mesh_idx + at, std::min(n - at, (int32_t)kMaxUpdatesPerLaunch), (hipStream_t)stream);
            if (e != HR_OK) return e;
        }
        return HR_OK;
    }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

hr_status hr_scene_device_rebuild_counts(const hr_scene* scene, int64_t* rebuilds_enqueued, int64_t* launches_enqueued)
{
    static const char* call = "hr_scene_device_rebuild_counts";
    if (!scene) return bad(call, "scene is NULL");
    if (!scene->deform) return bad(call, "not a scene from hr_scene_create_deformable or hr_scene_create_instanced_shared_deformable");
    if (rebuilds_enqueued) *rebuilds_enqueued = scene->redeals;
    if (launches_enqueued) *launches_enqueued = scene->redeal_launches;
    return HR_OK;
}

} // extern "C"
