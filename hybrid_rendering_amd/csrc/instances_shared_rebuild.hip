// hr_scene_rebuild_top_level_device: the top level of a shared instanced scene (instances_shared.hip) re-built on the GPU, kernels only on the
// caller's stream, nothing read back.  The SHAPE of the tree is fixed by the instance count (instance_math.h fixed_top_node: leaves dealt in
// order, as evenly as possible, to ceil(I / 8) bottom nodes, those grouped the same way up to the root), so the host writes the topology table
// once without ever seeing a box; what the device decides is the ORDER of the leaves: the instances sorted by the 30-bit Morton code of their
// world box's centre inside the bounds of the last update (instance_math.h sort_key: unique, so the order is a function of the boxes alone).
// Answers of a shared scene do not depend on the top level's topology (traverse2.h), so correctness never depends on this file's order.
//
//   (0) k_boxes_from_records    only when the device's instance boxes lag the records (no device update yet, or a host update since): box of
//                               every instance from the matrix its record holds, with the arithmetic of k_shared_records; the bounds the host knows
//   (1) sort                    I <= kSortSmall: k_sort_small, keys made and sorted in ONE workgroup's LDS (bitonic network, 64-bit keys);
//                               else k_keys, then per 8-bit digit of the code k_radix_hist / k_radix_scan / k_radix_scatter: a stable LSD radix
//                               sort of (code, instance) that starts from ascending instances, hence the same order as the 64-bit keys'
//   (2) k_gather                the records, in the new leaf order, into a scratch buffer (reads the old leaf_of)
//   (3) k_commit                scratch -> inst_shared (the passes hold that pointer), the new dev_leaf_inst / dev_leaf_of
//   (4) the refit               k_shared_top_one or the per-depth launches of instances_shared_update.hip over the fixed table; its last statement
//                               makes the half-area sum the new baseline of top_cost_ratio, clears the re-build flag and counts the re-build
//
// The two sorts live in device_sort.h (deform_redeal.hip uses them too), with the reasons for kSortSmall = 4096.  4096 instances is also about
// where the top level leaves the one-workgroup refit (kOneLaunchNodes = 1024 nodes: 4097 instances make 590), so "small" means the same thing in
// both files.
//
// Launches: 4 per re-build up to kSortSmall instances (+1 for (0)), else 1 + 12 + 2 + the refit's.  With a threshold set
// (hr_scene_set_device_rebuild_threshold) these launches ride behind EVERY device update, each one exiting at once unless the update's refit
// has set the status block's rebuild_flag: the host never learns whether a re-build ran, and need not — the shape is the same either way.
//
// A CAPTURED re-build re-orders the leaves at every replay, which this library never sees: the mirrors then count as stale before every host
// call, and the scene is marked order_replayed, on which the AO pass rebuilds its entry table at every render — the table holds top-level node
// indices, and the fixed shape keeps the slots but not the instances below them.
#include "instances_shared_device.h"
#include "device_sort.h"
#include <cmath>
#include <cstring>

using namespace hr;

namespace {

constexpr int kRecordWords = (int)(sizeof(InstanceShared) / 4);
static_assert(sizeof(InstanceShared) == 160, "InstanceShared layout");

__global__ void __launch_bounds__(256) k_boxes_from_records(const InstanceShared* records, const int32_t* leaf_of, const uint32_t* inst_mesh, const MeshTab* mesh,
                                                            float* inst_box, DeviceUpdateStatus* status, int n, const float lo0, const float lo1, const float lo2,
                                                            const float hi0, const float hi1, const float hi2, const float pad)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i == 0)
    {
        status->bounds[0] = lo0; status->bounds[1] = lo1; status->bounds[2] = lo2;
        status->bounds[3] = hi0; status->bounds[4] = hi1; status->bounds[5] = hi2;
        status->pad = pad; status->any_box = 1u;
    }
    if (i >= n) return;
    float m[16], box[6];
    const InstanceShared& r = records[leaf_of[i]];
    for (int k = 0; k < 16; k++) m[k] = r.m[k];
    imath::world_box(m, mesh[inst_mesh[i]].bounds, box);
    for (int k = 0; k < 6; k++) inst_box[(size_t)i * 6 + k] = box[k];
}

// blockDim.x == kSortLanes; n2: a power of two, n <= n2 <= kSortSmall
__global__ void __launch_bounds__(kSortLanes) k_sort_small(const float* inst_box, const DeviceUpdateStatus* status, uint32_t* order, int n, int n2, int predicated)
{
    __shared__ unsigned long long key[kSortSmall];
    if (rebuild_skipped(status, predicated)) return;
    const int t = (int)threadIdx.x;
    float bounds[6];
    for (int k = 0; k < 6; k++) bounds[k] = status->bounds[k];
    for (int e = t; e < n2; e += kSortLanes)
    {
        unsigned long long v = ~0ull;   // above every key: a code has 30 bits
        if (e < n)
        {
            float box[6];
            for (int k = 0; k < 6; k++) box[k] = inst_box[(size_t)e * 6 + k];
            v = imath::sort_key(box, bounds, (uint32_t)e);
        }
        key[e] = v;
    }
    __syncthreads();
    bitonic_sort_lds(key, n2, t);
    for (int e = t; e < n; e += kSortLanes) order[e] = (uint32_t)(key[e] & 0xffffffffull);
}

__global__ void __launch_bounds__(256) k_keys(const float* inst_box, const DeviceUpdateStatus* status, uint32_t* codes, uint32_t* idx, int n, int predicated)
{
    if (rebuild_skipped(status, predicated)) return;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    float bounds[6], box[6];
    for (int k = 0; k < 6; k++) { bounds[k] = status->bounds[k]; box[k] = inst_box[(size_t)i * 6 + k]; }
    codes[i] = imath::morton_code(box, bounds);
    idx[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_gather(const uint32_t* records, uint32_t* scratch, const uint32_t* order, const int32_t* leaf_of, const DeviceUpdateStatus* status,
                                                int n, int predicated)
{
    if (rebuild_skipped(status, predicated)) return;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)n * kRecordWords) return;
    const int l = (int)(g / kRecordWords), w = (int)(g % kRecordWords);
    const uint32_t inst = order[l];
    if (inst >= (uint32_t)n) return;
    const int32_t from = leaf_of[inst];
    if ((uint32_t)from >= (uint32_t)n) return;
    scratch[g] = records[(size_t)from * kRecordWords + w];
}

__global__ void __launch_bounds__(256) k_commit(uint32_t* records, const uint32_t* scratch, const uint32_t* order, int32_t* leaf_inst, int32_t* leaf_of,
                                                const DeviceUpdateStatus* status, int n, int predicated)
{
    if (rebuild_skipped(status, predicated)) return;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)n * kRecordWords) return;
    records[g] = scratch[g];
    if (g < n)
    {
        const uint32_t inst = order[g];
        if (inst < (uint32_t)n) { leaf_inst[g] = (int32_t)inst; leaf_of[inst] = (int32_t)g; }
    }
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

hr_status ensure_buffers(hr_scene* s)
{
    SharedDeviceUpdate& du = *s->dev_update;
    if (du.rebuild_ready) return HR_OK;
    const size_t I = (size_t)s->n_instances;
    hr_status e;
    for (int k = 0; k < 2; k++)
    {
        if ((e = du.rb_codes[k].alloc(I * 4)) != HR_OK) return e;
        if ((e = du.rb_idx[k].alloc(I * 4)) != HR_OK) return e;
    }
    if ((e = du.rb_hist.alloc(radix_hist_bytes(I))) != HR_OK) return e;
    if ((e = du.rb_records.alloc(I * sizeof(InstanceShared))) != HR_OK) return e;
    du.rebuild_ready = true;
    return HR_OK;
}

// the host side of the fixed shape: the table, the depth ranges, one copy
hr_status adopt_fixed_shape(hr_scene* s, hipStream_t st, const char* call)
{
    const int I = s->n_instances;
    const int n_nodes = imath::fixed_top_nodes(I), n_depths = imath::fixed_top_depths(I);
    if (n_nodes > s->top_cap) { set_last_error(std::string(call) + ": the fixed top level does not fit the slots reserved for the top level"); return HR_ERR_UNSUPPORTED; }
    if (n_depths - 1 + s->shared_mesh_depth + 2 >= kMaxTraversalDepth) { set_last_error(std::string(call) + ": top level + deepest mesh tree exceed the traversal stack"); return HR_ERR_UNSUPPORTED; }
    {
        const hr_status ws = instanced_scene_wait_uploads(s);   // shared_top may still feed an earlier call's copy
        if (ws != HR_OK) return ws;
    }
    s->shared_top.resize((size_t)n_nodes);
    s->shared_depth_start.assign((size_t)n_depths + 1, 0);
    for (int d = 0; d <= n_depths; d++) s->shared_depth_start[(size_t)d] = imath::fixed_top_depth_start(I, d);
    for (int d = 0; d < n_depths; d++)
        for (int j = 0; j < s->shared_depth_start[(size_t)d + 1] - s->shared_depth_start[(size_t)d]; j++)
            s->shared_top[(size_t)s->shared_depth_start[(size_t)d] + j] = imath::fixed_top_node(I, d, j);
    HR_HIP(hipMemcpyAsync(s->dev_top.p, s->shared_top.data(), (size_t)n_nodes * sizeof(SharedTopNode), hipMemcpyHostToDevice, st));
    // slots the fixed shape leaves unused read as empty nodes, as they do after a host re-build (nothing references them)
    if (n_nodes < s->top_cap) HR_HIP(hipMemsetAsync((Node8*)s->nodes.p + n_nodes, 0, (size_t)(s->top_cap - n_nodes) * sizeof(Node8), st));
    {
        const hr_status ms = instanced_scene_mark_uploads(s, st);
        if (ms != HR_OK) return ms;
    }
    s->info.max_depth = n_depths - 1 + 1 + s->shared_mesh_depth;
    s->fixed_shape = true;
    return HR_OK;
}

hr_status scene_check(const hr_scene* s, const char* call)
{
    if (!s) return bad(call, "scene is NULL");
    if (!s->shared) return bad(call, "not a shared instanced scene (hr_scene_create_instanced_shared)");
    return HR_OK;
}

} // namespace

namespace {

// every launch of one re-build, (0) to (4)
hr_status enqueue_launches(hr_scene* s, hipStream_t st, bool counted, bool predicated, bool capturing)
{
    SharedDeviceUpdate& du = *s->dev_update;
    const int I = s->n_instances, pred = predicated ? 1 : 0;
    DeviceUpdateStatus* status = (DeviceUpdateStatus*)du.status.p;
    const float* inst_box = (const float*)du.inst_box.p;
    int64_t launched = 0;
    if (!du.boxes_current)
    {
        const float pad = imath::pad_of_bounds(s->grid_lo, s->grid_hi);
        hipLaunchKernelGGL(k_boxes_from_records, dim3(cdiv(I, 256)), dim3(256), 0, st, (const InstanceShared*)s->inst_shared.p, (const int32_t*)s->dev_leaf_of.p,
                           (const uint32_t*)s->dev_inst_mesh.p, (const MeshTab*)s->dev_mesh_tab.p, (float*)du.inst_box.p, status, I,
                           s->grid_lo[0], s->grid_lo[1], s->grid_lo[2], s->grid_hi[0], s->grid_hi[1], s->grid_hi[2], pad);
        HR_HIP(hipGetLastError());
        launched++;
        // a captured launch has not run: the boxes stay stale for every eager call until a replay or an update makes them (the captured one
        // carries the bounds and the pad the host knows NOW into every replay: INTEGRATION.md)
        if (!capturing) du.boxes_current = true;
    }
    uint32_t* order = (uint32_t*)du.rb_idx[0].p;
    if (I <= kSortSmall)
    {
        int n2 = 64;
        while (n2 < I) n2 *= 2;
        hipLaunchKernelGGL(k_sort_small, dim3(1), dim3(kSortLanes), 0, st, inst_box, status, order, I, n2, pred);
        HR_HIP(hipGetLastError());
        launched++;
    }
    else
    {
        hipLaunchKernelGGL(k_keys, dim3(cdiv(I, 256)), dim3(256), 0, st, inst_box, status, (uint32_t*)du.rb_codes[0].p, (uint32_t*)du.rb_idx[0].p, I, pred);
        HR_HIP(hipGetLastError());
        launched++;
        uint32_t* const codes[2] = { (uint32_t*)du.rb_codes[0].p, (uint32_t*)du.rb_codes[1].p };
        uint32_t* const idx[2]   = { (uint32_t*)du.rb_idx[0].p, (uint32_t*)du.rb_idx[1].p };
        const hr_status rs = radix_sort_enqueue(codes, idx, (uint32_t*)du.rb_hist.p, status, I, pred, st, &launched);   // the order ends in rb_idx[0]
        if (rs != HR_OK) return rs;
    }
    const int word_blocks = (int)(((long long)I * kRecordWords + 255) / 256);
    hipLaunchKernelGGL(k_gather, dim3(word_blocks), dim3(256), 0, st, (const uint32_t*)s->inst_shared.p, (uint32_t*)du.rb_records.p, (const uint32_t*)order,
                       (const int32_t*)s->dev_leaf_of.p, status, I, pred);
    HR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_commit, dim3(word_blocks), dim3(256), 0, st, (uint32_t*)s->inst_shared.p, (const uint32_t*)du.rb_records.p, (const uint32_t*)order,
                       (int32_t*)s->dev_leaf_inst.p, (int32_t*)s->dev_leaf_of.p, status, I, pred);
    HR_HIP(hipGetLastError());
    launched += 2;
    du.launches += launched; du.rebuild_launches += launched;
    return shared_device_refit_enqueue(s, st, counted ? kRefitRebuildCounted : kRefitRebuildQuiet, predicated);
}

} // namespace

hr_status hr::shared_device_rebuild_enqueue(hr_scene* s, hipStream_t st, const char* call, bool counted, bool predicated)
{
    HR_HIP(hipSetDevice(s->ctx->device));
    const bool capturing = stream_is_capturing(st);
    if (!s->fixed_shape && capturing)
        return bad(call, "the first device re-build changes the top level's shape and uploads it: not possible while the stream is capturing (re-build once before the capture)");
    hr_status e;
    if ((e = shared_device_work_ensure(s)) != HR_OK) return e;
    SharedDeviceUpdate& du = *s->dev_update;
    if (!du.rebuild_ready && capturing) return bad(call, "the first device re-build allocates: not possible while the stream is capturing");
    if ((e = ensure_buffers(s)) != HR_OK) return e;
    if (!s->fixed_shape && (e = adopt_fixed_shape(s, st, call)) != HR_OK) return e;   // the refit below reads the host's table: it has to stand first
    e = enqueue_launches(s, st, counted, predicated, capturing);
    // Also after an error: some launches may be in the stream, and the table may be the fixed one over nodes of the old shape.  The mirrors
    // and the passes' caches count as stale either way; what the error leaves is undefined until a re-build of either kind succeeds.
    du.status_stale = true;
    du.last_stream = st;
    du.captured = du.captured || capturing;   // replays re-order the leaves unseen: the mirrors count as stale before every host call
    s->order_replayed = s->order_replayed || capturing;
    s->mirrors_stale = true;
    s->geometry_epoch++;
    if (e != HR_OK)
    {
        du.boxes_current = false;
        set_last_error(std::string(hr_last_error()) + " (" + call + ": the scene's top level is undefined until a re-build succeeds)");
        return e;
    }
    du.device_baseline = true;
    return HR_OK;
}

extern "C" {

hr_status hr_shared_top_fixed_shape(int32_t n_instances, void* nodes_out, int64_t capacity, int32_t* n_nodes, int32_t* n_depths)
{
    static const char* call = "hr_shared_top_fixed_shape";
    if (n_instances < 1) return bad(call, "n_instances < 1");
    const int n = imath::fixed_top_nodes(n_instances), D = imath::fixed_top_depths(n_instances);
    if (n_nodes) *n_nodes = n;
    if (n_depths) *n_depths = D;
    if (!nodes_out) return HR_OK;
    if (capacity < (int64_t)n) return bad(call, "capacity is below the node count");
    SharedTopNode* out = (SharedTopNode*)nodes_out;
    for (int d = 0; d < D; d++)
    {
        const int first = imath::fixed_top_depth_start(n_instances, d), count = imath::fixed_top_depth_start(n_instances, d + 1) - first;
        for (int j = 0; j < count; j++) out[first + j] = imath::fixed_top_node(n_instances, d, j);
    }
    return HR_OK;
}

hr_status hr_shared_top_sort_keys(const float* inst_boxes, int32_t n, const float bounds[6], uint64_t* keys_out)
{
    static const char* call = "hr_shared_top_sort_keys";
    if (n < 0 || (n > 0 && (!inst_boxes || !keys_out)) || !bounds) return bad(call, "NULL argument or n < 0");
    for (int32_t i = 0; i < n; i++) keys_out[i] = imath::sort_key(inst_boxes + (size_t)i * 6, bounds, (uint32_t)i);
    return HR_OK;
}

hr_status hr_scene_rebuild_top_level_device(hr_scene* scene, void* stream)
{
    static const char* call = "hr_scene_rebuild_top_level_device";
    try
    {
        const hr_status c = scene_check(scene, call);
        if (c != HR_OK) return c;
        return shared_device_rebuild_enqueue(scene, (hipStream_t)stream, call, true, false);
    }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

hr_status hr_scene_set_device_rebuild_threshold(hr_scene* scene, float ratio, void* stream)
{
    static const char* call = "hr_scene_set_device_rebuild_threshold";
    try
    {
        const hr_status c = scene_check(scene, call);
        if (c != HR_OK) return c;
        if (ratio == 0.0f)
        {
            if (scene->dev_update) scene->dev_update->threshold = 0.0f;
            return HR_OK;
        }
        if (!(ratio > 1.0f) || !std::isfinite(ratio)) return bad(call, "ratio must be 0 (off) or a finite value above 1");
        // onto the fixed shape at once, over a fresh order: the baseline the threshold compares against (not counted as a re-build)
        const hr_status e = shared_device_rebuild_enqueue(scene, (hipStream_t)stream, call, false, false);
        if (e != HR_OK) return e;
        scene->dev_update->threshold = ratio;
        return HR_OK;
    }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

hr_status hr_scene_device_rebuild_status(const hr_scene* scene, int64_t* rebuilds_done, int64_t* launches_enqueued, int32_t* fixed_shape)
{
    static const char* call = "hr_scene_device_rebuild_status";
    const hr_status c = scene_check(scene, call);
    if (c != HR_OK) return c;
    int64_t done = 0, launches = 0;
    if (scene->dev_update)
    {
        const hr_status w = shared_device_status_refresh(scene);
        if (w != HR_OK) return w;
        done = (int64_t)((const DeviceUpdateStatus*)scene->dev_update->status_host)->rebuilds_done;
        launches = scene->dev_update->rebuild_launches;
    }
    if (rebuilds_done) *rebuilds_done = done;
    if (launches_enqueued) *launches_enqueued = launches;
    if (fixed_shape) *fixed_shape = scene->fixed_shape ? 1 : 0;
    return HR_OK;
}

} // extern "C"
