// hr_scene_update_instances_device: the per-frame update of a shared instanced scene (instances_shared.hip) from matrices that live in DEVICE
// memory.  Nothing is built: the top level's topology stays as the host last made it; the instance records, the instances' world boxes and the
// top level's boxes are recomputed by two kernels with the arithmetic of the host path (instance_math.h: one body for both, so the records and the
// nodes equal the host path's bit for bit).
//
//   (a) k_shared_records        one lane per instance: matrix -> record (written into the instance's LEAF slot, only when the matrix changed and is
//                               finite) and world box (always, from the matrix the record holds afterwards); the scene's bounds folded per wave
//                               with one atomic per wave and component when they are measured; non-finite matrices and boxes outside given bounds
//                               counted the same way.
//   (b) k_shared_top_one        the whole top level in ONE workgroup, one lane per node: the deepest depth first, __syncthreads() between depths,
//                               the node boxes in LDS; then one fixed-order sum of the nodes' half areas (what the re-build trigger looks at).
//       k_shared_top_depth /    larger top levels: one launch per depth (slots are breadth-first: a depth is a contiguous slot range), node boxes
//       k_shared_top_root       in global memory; the root's launch also sums the areas.
//
// Launches per update: kLaunchesSmall = 2 when the top level has at most kOneLaunchNodes = 1024 nodes — about 5000 instances, a node holding up
// to 8 children — else 1 + the top level's depth count.  1024 is one lane per node at the largest workgroup the hardware schedules (16 waves):
// 24 bytes of LDS per node for its box plus 8 for its area make 32 KiB, far inside a CU's LDS, and the cost is one barrier per depth instead of
// one launch plus a global round trip per depth.  The work is latency-bound; occupancy is of no interest (one workgroup runs).
//
// The pad of the leaf boxes is 3e-5 x the diagonal of the scene's bounds: a kernel argument when the caller gives the bounds, computed from the
// accumulated bounds on the device when they are measured (then the call waits once, for the status block, so that the host's grid_lo / grid_hi and
// info follow).  The accumulators are consumed and reset by (b)'s last workgroup, so no launch is spent on clearing them.
//
// The refit (b) is also the tail of the device re-build of the top level (instances_shared_rebuild.hip, which sorts the leaves into a tree of
// fixed shape): there it takes the last update's bounds and pad from the status block, makes its half-area sum the baseline top_cost_ratio is
// relative to, and clears rebuild_flag — the flag an update's refit sets when a threshold is on and area / baseline exceeds it, and on which
// the re-build's launches behind that update are predicated.
#include "instances_shared_device.h"
#include <cmath>
#include <cstring>

using namespace hr;

namespace {

constexpr int kOneLaunchNodes = 1024;
constexpr int kLaunchesSmall  = 2;

constexpr uint32_t kAccLoInit = 0xffffffffu, kAccHiInit = 0u;

__host__ __device__ inline uint32_t ordered_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return (u >> 31) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float    ordered_value(uint32_t o) { const uint32_t u = (o >> 31) ? (o & 0x7fffffffu) : ~o; float f; __builtin_memcpy(&f, &u, 4); return f; }

struct RecordArgs
{
    const float*    mats;
    InstanceShared* records;
    const int32_t*  leaf_of;
    const uint32_t* inst_mesh;
    const MeshTab*  mesh;
    float*          inst_box;
    DeviceUpdateStatus* status;
    int             n;
    int             given;       // bounds given by the caller: check the boxes against them instead of measuring
    float           lo[3], hi[3];
};

__global__ void __launch_bounds__(256) k_shared_records(const RecordArgs a)
{
    const int  i    = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool live = i < a.n;
    bool  rejected = false, outside = false, counts = false;
    float box[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    if (live)
    {
        float m[16];
        for (int k = 0; k < 16; k++) m[k] = a.mats[(size_t)i * 16 + k];
        InstanceShared& r = a.records[a.leaf_of[i]];
        const MeshTab&  mt = a.mesh[a.inst_mesh[i]];
        bool same = true;
        for (int k = 0; k < 16; k++) same = same && __float_as_uint(m[k]) == __float_as_uint(r.m[k]);
        rejected = !imath::finite16(m);
        if (rejected)
            for (int k = 0; k < 16; k++) m[k] = r.m[k];   // the instance keeps its record; its box follows the standing matrix
        else if (!same)
        {
            float inv[9], iar[3], extent;
            uint32_t flags;
            imath::record_terms(m, mt.absmax, inv, iar, &extent, &flags);
            for (int k = 0; k < 16; k++) r.m[k] = m[k];
            for (int k = 0; k < 9; k++) r.inv[k] = inv[k];
            for (int k = 0; k < 3; k++) r.inv_abs_row[k] = iar[k];
            r.extent = extent; r.flags = (r.flags & kInstanceMaskBits) | flags;   // the instance's mask stays
        }
        imath::world_box(m, mt.bounds, box);
        for (int k = 0; k < 6; k++) a.inst_box[(size_t)i * 6 + k] = box[k];
        counts = mt.bounds[0] <= mt.bounds[3];   // an empty mesh's point box is no part of the scene's bounds (instances.hip instance_boxes)
        if (!counts) for (int k = 0; k < 3; k++) { box[k] = INFINITY; box[3 + k] = -INFINITY; }
        if (a.given && counts)
            for (int k = 0; k < 3; k++) outside = outside || !(box[k] >= a.lo[k]) || !(box[3 + k] <= a.hi[k]);
    }
    // one atomic per wave and quantity
    const unsigned long long rej = __ballot(rejected), out = __ballot(outside), cnt = __ballot(counts);
    if (!a.given)
        for (int off = 32; off > 0; off >>= 1)
            for (int k = 0; k < 3; k++)
            {
                box[k]     = imath::fmin_(box[k], __shfl_xor(box[k], off));
                box[3 + k] = imath::fmax_(box[3 + k], __shfl_xor(box[3 + k], off));
            }
    if ((threadIdx.x & 63) == 0)
    {
        if (rej) atomicAdd(&a.status->acc_rejected, (uint32_t)__popcll(rej));
        if (out) atomicOr(&a.status->acc_violated, 1u);
        if (!a.given && cnt)
            for (int k = 0; k < 3; k++) { atomicMin(&a.status->acc_lo[k], ordered_bits(box[k])); atomicMax(&a.status->acc_hi[k], ordered_bits(box[3 + k])); }
    }
}

struct TopArgs
{
    const SharedTopNode* top;
    const int32_t*       leaf_inst;
    const float*         inst_box;
    Node8*               nodes;
    float*               node_box;   // global node boxes (the per-depth path)
    double*              areas;
    DeviceUpdateStatus*  status;
    int                  n_nodes, n_depths;
    int                  first, count;   // the per-depth path: this launch's slot range
    int                  given;
    float                pad;            // given bounds: the pad they make
    float                lo[3], hi[3];   // given bounds
    int                  mode;           // kRefitUpdate, or the tail of a device re-build: bounds and pad are the status block's
    int                  predicated;     // run only when the status block's rebuild_flag is set
    float                ratio;          // kRefitUpdate: the re-build threshold (0: off)
};

// the pad of this update: the argument, or made from the bounds (a) accumulated
__device__ inline float pad_of_update(const TopArgs& a, float* lo, float* hi, bool* any)
{
    if (a.mode != kRefitUpdate)
    {
        for (int k = 0; k < 3; k++) { lo[k] = a.status->bounds[k]; hi[k] = a.status->bounds[3 + k]; }
        *any = a.status->any_box != 0u;
        return a.status->pad;
    }
    if (a.given)
    {
        for (int k = 0; k < 3; k++) { lo[k] = a.lo[k]; hi[k] = a.hi[k]; }
        *any = true;
        return a.pad;
    }
    bool some = true;
    for (int k = 0; k < 3; k++)
    {
        const uint32_t l = a.status->acc_lo[k], h = a.status->acc_hi[k];
        lo[k] = ordered_value(l); hi[k] = ordered_value(h);
        some = some && l != kAccLoInit && !(lo[k] > hi[k]);
    }
    if (!some) for (int k = 0; k < 3; k++) { lo[k] = 0.0f; hi[k] = 0.0f; }   // no instance with geometry
    *any = some;
    return imath::pad_of_bounds(lo, hi);
}

// one node from its children's boxes (`box`: LDS or global, 6 floats per slot); returns its half area
__device__ inline double refit_slot(const TopArgs& a, int slot, float pad, float* box)
{
    const SharedTopNode t = a.top[slot];
    const int nc = t.n_internal + t.n_leaves;
    float clo[8][3], chi[8][3], lo[3], hi[3];
    for (int c = 0; c < nc; c++)
        for (int k = 0; k < 3; k++)
        {
            if (c < t.n_internal) { clo[c][k] = box[((size_t)t.child_base + c) * 6 + k]; chi[c][k] = box[((size_t)t.child_base + c) * 6 + 3 + k]; }
            else
            {
                const float* b = &a.inst_box[(size_t)a.leaf_inst[t.leaf_base + (c - t.n_internal)] * 6];
                clo[c][k] = b[k] - pad; chi[c][k] = b[3 + k] + pad;
            }
        }
    Node8 nd;
    const double area = imath::top_node(t, clo, chi, nd, lo, hi);
    a.nodes[slot] = nd;
    for (int k = 0; k < 3; k++) { box[(size_t)slot * 6 + k] = lo[k]; box[(size_t)slot * 6 + 3 + k] = hi[k]; }
    return area;
}

// ONE fixed-order sum (lane t takes its partial, then a halving tree in LDS), then the status block: results out, accumulators reset
__device__ inline void finish_update(const TopArgs& a, double partial, double* red, const float* lo, const float* hi, float pad, bool any)
{
    const int t = (int)threadIdx.x;
    red[t] = partial;
    __syncthreads();
    for (int s = (int)blockDim.x >> 1; s > 0; s >>= 1)
    {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0)
    {
        DeviceUpdateStatus* st = a.status;
        if (a.mode != kRefitUpdate)   // a re-build's tail: the area is the new baseline; the last update's bounds and counts stand
        {
            st->area = red[0]; st->baseline = red[0]; st->rebuild_flag = 0u;
            if (a.mode == kRefitRebuildCounted) st->rebuilds_done++;
            return;
        }
        st->rebuild_flag = (a.ratio > 0.0f && st->baseline > 0.0 && red[0] / st->baseline > (double)a.ratio) ? 1u : 0u;   // threshold off: always clear
        for (int k = 0; k < 3; k++) { st->bounds[k] = lo[k]; st->bounds[3 + k] = hi[k]; }
        st->pad = pad; st->any_box = any ? 1u : 0u;
        st->rejected = st->acc_rejected; st->violated = st->acc_violated;
        st->area = red[0];
        for (int k = 0; k < 3; k++) { st->acc_lo[k] = kAccLoInit; st->acc_hi[k] = kAccHiInit; }
        st->acc_rejected = 0u; st->acc_violated = 0u;
    }
}

// blockDim.x: a power of two >= n_nodes, <= kOneLaunchNodes
__global__ void __launch_bounds__(kOneLaunchNodes) k_shared_top_one(const TopArgs a)
{
    __shared__ float  box[kOneLaunchNodes * 6];
    __shared__ double red[kOneLaunchNodes];
    if (a.predicated && a.status->rebuild_flag == 0u) return;   // the whole workgroup: the flag changes in this kernel's last statement only
    const int slot = (int)threadIdx.x;
    float lo[3], hi[3];
    bool  any;
    const float pad = pad_of_update(a, lo, hi, &any);
    const int   my_depth = slot < a.n_nodes ? a.top[slot].depth : -1;
    double area = 0.0;
    for (int d = a.n_depths - 1; d >= 0; d--)
    {
        if (my_depth == d) area = refit_slot(a, slot, pad, box);
        __syncthreads();
    }
    finish_update(a, area, red, lo, hi, pad, any);
}

__global__ void __launch_bounds__(256) k_shared_top_depth(const TopArgs a)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= a.count) return;
    if (a.predicated && a.status->rebuild_flag == 0u) return;   // cleared by the root's launch, behind every depth's
    float lo[3], hi[3];
    bool  any;
    const float pad = pad_of_update(a, lo, hi, &any);
    a.areas[a.first + j] = refit_slot(a, a.first + j, pad, a.node_box);
}

// the root (slot 0, the last depth to be refitted) and the sum; one workgroup of kOneLaunchNodes lanes
__global__ void __launch_bounds__(kOneLaunchNodes) k_shared_top_root(const TopArgs a)
{
    __shared__ double red[kOneLaunchNodes];
    if (a.predicated && a.status->rebuild_flag == 0u) return;
    float lo[3], hi[3];
    bool  any;
    const float pad = pad_of_update(a, lo, hi, &any);
    double partial = 0.0;
    if (threadIdx.x == 0) partial = refit_slot(a, 0, pad, a.node_box);
    for (int j = (int)threadIdx.x; j < a.n_nodes; j += (int)blockDim.x)
        if (j != 0) partial += a.areas[j];   // ascending slots per lane: a fixed order
    finish_update(a, partial, red, lo, hi, pad, any);
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

} // namespace

bool hr::stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const hipError_t ce = hipStreamIsCapturing(st, &cap);
    if (ce != hipSuccess) (void)hipGetLastError();
    return ce != hipSuccess || cap != hipStreamCaptureStatusNone;
}

hr_status hr::shared_device_work_ensure(hr_scene* s)
{
    if (s->dev_update) return HR_OK;
    std::unique_ptr<SharedDeviceUpdate> du(new SharedDeviceUpdate());
    const size_t I = (size_t)s->n_instances;
    hr_status e;
    if ((e = du->inst_box.alloc(I * 24)) != HR_OK) return e;
    if ((e = du->node_box.alloc((size_t)s->top_cap * 24)) != HR_OK) return e;
    if ((e = du->areas.alloc((size_t)s->top_cap * 8)) != HR_OK) return e;
    if ((e = du->status.alloc(sizeof(DeviceUpdateStatus))) != HR_OK) return e;
    HR_HIP(hipHostMalloc(&du->status_host, sizeof(DeviceUpdateStatus), hipHostMallocDefault));
    DeviceUpdateStatus init;
    std::memset(&init, 0, sizeof(init));
    for (int k = 0; k < 3; k++) { init.acc_lo[k] = kAccLoInit; init.acc_hi[k] = kAccHiInit; }
    std::memcpy(du->status_host, &init, sizeof(init));
    HR_HIP(hipMemcpy(du->status.p, &init, sizeof(init), hipMemcpyHostToDevice));
    s->dev_update = std::move(du);
    return HR_OK;
}

// the top level's refit over the scene's standing topology: one workgroup up to kOneLaunchNodes nodes, else one launch per depth
static hr_status refit_enqueue(hr_scene* s, hipStream_t st, const float* bounds, int mode, bool predicated)
{
    SharedDeviceUpdate& du = *s->dev_update;
    const int n_nodes = (int)s->shared_top.size(), n_depths = (int)s->shared_depth_start.size() - 1;
    TopArgs ta;
    ta.top = (const SharedTopNode*)s->dev_top.p; ta.leaf_inst = (const int32_t*)s->dev_leaf_inst.p; ta.inst_box = (const float*)du.inst_box.p;
    ta.nodes = (Node8*)s->nodes.p; ta.node_box = (float*)du.node_box.p; ta.areas = (double*)du.areas.p; ta.status = (DeviceUpdateStatus*)du.status.p;
    ta.n_nodes = n_nodes; ta.first = 0; ta.count = n_nodes; ta.given = bounds ? 1 : 0;
    ta.pad = bounds ? imath::pad_of_bounds(bounds, bounds + 3) : 0.0f;
    for (int k = 0; k < 3; k++) { ta.lo[k] = bounds ? bounds[k] : 0.0f; ta.hi[k] = bounds ? bounds[3 + k] : 0.0f; }
    ta.mode = mode; ta.predicated = predicated ? 1 : 0; ta.ratio = mode == kRefitUpdate ? du.threshold : 0.0f;
    const int* start = s->shared_depth_start.data();   // slots are breadth-first: depth d is the slot range [start[d], start[d + 1])
    ta.n_depths = n_depths;
    int64_t launched = 0;
    if (n_nodes <= kOneLaunchNodes)
    {
        int threads = 64;
        while (threads < n_nodes) threads *= 2;
        hipLaunchKernelGGL(k_shared_top_one, dim3(1), dim3(threads), 0, st, ta);
        HR_HIP(hipGetLastError());
        launched++;
    }
    else
    {
        for (int d = n_depths - 1; d >= 1; d--)
        {
            ta.first = start[d]; ta.count = start[d + 1] - start[d];
            hipLaunchKernelGGL(k_shared_top_depth, dim3(cdiv(ta.count, 256)), dim3(256), 0, st, ta);
            HR_HIP(hipGetLastError());
            launched++;
        }
        ta.first = 0; ta.count = 1;
        hipLaunchKernelGGL(k_shared_top_root, dim3(1), dim3(kOneLaunchNodes), 0, st, ta);
        HR_HIP(hipGetLastError());
        launched++;
    }
    du.launches += launched;
    if (mode != kRefitUpdate) du.rebuild_launches += launched;
    return HR_OK;
}

hr_status hr::shared_device_refit_enqueue(hr_scene* s, hipStream_t st, int mode, bool predicated) { return refit_enqueue(s, st, nullptr, mode, predicated); }

namespace {

hr_status update_device_impl(hr_scene* s, const float* mats, const float* bounds, hipStream_t st)
{
    static const char* call = "hr_scene_update_instances_device";
    if (!s) return bad(call, "scene is NULL");
    if (!s->shared) return bad(call, "not a shared instanced scene (hr_scene_create_instanced_shared)");
    if (!mats) return bad(call, "model_matrices is NULL");
    if (bounds)
    {
        for (int k = 0; k < 6; k++) if (!std::isfinite(bounds[k])) return bad(call, "world_bounds are not finite");
        for (int k = 0; k < 3; k++) if (bounds[k] > bounds[3 + k]) return bad(call, "world_bounds have lo > hi");
    }
    HR_HIP(hipSetDevice(s->ctx->device));
    const bool capturing = stream_is_capturing(st);
    if (capturing && !bounds)
        return bad(call, "world_bounds == NULL measures the bounds and waits for them: not possible while the stream is capturing (give the bounds)");
    const int n_depths = (int)s->shared_depth_start.size() - 1;   // shared_device_tables_upload: checked and laid out where the top level is adopted
    if (n_depths < 1 || s->shared_depth_start[(size_t)n_depths] != (int)s->shared_top.size()) return bad(call, "the scene has no device copy of its top level");
    {
        const hr_status e = shared_device_work_ensure(s);
        if (e != HR_OK) return e;
    }
    SharedDeviceUpdate& du = *s->dev_update;
    const bool thresholded = du.threshold > 0.0f;
    if (thresholded && !s->fixed_shape)   // a host re-build took the scene off the fixed shape since the threshold was set: back onto it first
    {
        const hr_status e = shared_device_rebuild_enqueue(s, st, call, false, false);
        if (e != HR_OK) return e;
    }
    const int I = s->n_instances;

    RecordArgs ra;
    ra.mats = mats; ra.records = (InstanceShared*)s->inst_shared.p; ra.leaf_of = (const int32_t*)s->dev_leaf_of.p;
    ra.inst_mesh = (const uint32_t*)s->dev_inst_mesh.p; ra.mesh = (const MeshTab*)s->dev_mesh_tab.p; ra.inst_box = (float*)du.inst_box.p;
    ra.status = (DeviceUpdateStatus*)du.status.p; ra.n = I; ra.given = bounds ? 1 : 0;
    for (int k = 0; k < 3; k++) { ra.lo[k] = bounds ? bounds[k] : 0.0f; ra.hi[k] = bounds ? bounds[3 + k] : 0.0f; }
    hipLaunchKernelGGL(k_shared_records, dim3(cdiv(I, 256)), dim3(256), 0, st, ra);
    HR_HIP(hipGetLastError());
    du.launches++;

    {
        const hr_status e = refit_enqueue(s, st, bounds, kRefitUpdate, false);
        if (e != HR_OK) return e;
    }
    du.boxes_current = true;
    du.given_bounds = bounds != nullptr;
    du.area_at_build = s->top_area_at_build;
    du.status_stale = true;
    du.last_stream = st;
    // a captured update runs again at every replay, on a stream and at a time this library never sees: from here on the status is read back on
    // every status call and the host mirrors count as stale before every host call
    du.captured = du.captured || capturing;
    s->mirrors_stale = true;
    if (bounds)
    {
        for (int k = 0; k < 3; k++) { s->grid_lo[k] = bounds[k]; s->grid_hi[k] = bounds[3 + k]; }
    }
    else
    {
        HR_HIP(hipMemcpyAsync(du.status_host, du.status.p, sizeof(DeviceUpdateStatus), hipMemcpyDeviceToHost, st));
        HR_HIP(hipStreamSynchronize(st));   // the one wait of this call: the host's bounds (grid_lo / grid_hi, info) follow the measured ones
        du.stream_waits++;
        du.status_stale = false;
        const DeviceUpdateStatus* hs = (const DeviceUpdateStatus*)du.status_host;
        for (int k = 0; k < 3; k++) { s->grid_lo[k] = hs->bounds[k]; s->grid_hi[k] = hs->bounds[3 + k]; }
    }
    s->info.box_pad = imath::pad_of_bounds(s->grid_lo, s->grid_hi);
    for (int a = 0; a < 3; a++) { s->info.bounds_lo[a] = s->grid_lo[a]; s->info.bounds_hi[a] = s->grid_hi[a]; }
    s->geometry_epoch++;
    // the threshold mode: the re-build rides behind every update, its launches predicated on the flag the refit above has just written
    if (thresholded) return shared_device_rebuild_enqueue(s, st, call, true, true);
    return HR_OK;
}

} // namespace

hr_status hr::shared_device_mesh_table_upload(hr_scene* s, hipStream_t st)
{
    const size_t M = s->mesh_bounds.size() / 6;
    if (!s->dev_mesh_tab.p) { const hr_status e = s->dev_mesh_tab.alloc(M * sizeof(MeshTab)); if (e != HR_OK) return e; }
    s->mesh_tab_host.assign(M * 12, 0.0f);
    for (size_t k = 0; k < M; k++)
    {
        MeshTab t;
        std::memset(&t, 0, sizeof(t));
        for (int a = 0; a < 6; a++) t.bounds[a] = s->mesh_bounds[k * 6 + a];
        for (int a = 0; a < 3; a++) t.absmax[a] = s->shared_mesh_absmax[k * 3 + a];
        t.root = s->shared_mesh_root[k];
        t.tri_base = k < s->shared_mesh_tri_base.size() ? s->shared_mesh_tri_base[k] : 0u;
        std::memcpy(&s->mesh_tab_host[k * 12], &t, sizeof(t));
    }
    HR_HIP(hipMemcpyAsync(s->dev_mesh_tab.p, s->mesh_tab_host.data(), M * sizeof(MeshTab), hipMemcpyHostToDevice, st));
    return HR_OK;
}

hr_status hr::shared_device_tables_upload(hr_scene* s, hipStream_t st, bool all)
{
    const size_t I = (size_t)s->n_instances;
    static_assert(sizeof(SharedTopNode) == 24, "SharedTopNode layout");
    if (!s->dev_top.p)
    {
        hr_status e;
        if ((e = s->dev_top.alloc((size_t)s->top_cap * sizeof(SharedTopNode))) != HR_OK) return e;
        if ((e = s->dev_leaf_inst.alloc(I * 4)) != HR_OK) return e;
        if ((e = s->dev_leaf_of.alloc(I * 4)) != HR_OK) return e;
        if ((e = s->dev_inst_mesh.alloc(I * 4)) != HR_OK) return e;
    }
    if (s->shared_top.size() > (size_t)s->top_cap || s->shared_leaf_inst.size() != I || s->shared_leaf_of.size() != I)
    {
        set_last_error("shared scene: the top level does not fit the slots reserved for it");
        return HR_ERR_UNSUPPORTED;
    }
    HR_HIP(hipMemcpyAsync(s->dev_top.p, s->shared_top.data(), s->shared_top.size() * sizeof(SharedTopNode), hipMemcpyHostToDevice, st));
    HR_HIP(hipMemcpyAsync(s->dev_leaf_inst.p, s->shared_leaf_inst.data(), I * 4, hipMemcpyHostToDevice, st));
    HR_HIP(hipMemcpyAsync(s->dev_leaf_of.p, s->shared_leaf_of.data(), I * 4, hipMemcpyHostToDevice, st));
    // the slot range of every depth: what the refit launches walk, deepest first
    s->shared_depth_start.clear();
    for (size_t j = 0; j < s->shared_top.size(); j++)
    {
        const int d = s->shared_top[j].depth, have = (int)s->shared_depth_start.size();
        if (d < 0 || d > kMaxTraversalDepth || d < have - 1 || d > have) { set_last_error("shared scene: the top level's slots are not in depth order"); return HR_ERR_UNSUPPORTED; }
        if (d == have) s->shared_depth_start.push_back((int)j);
    }
    s->shared_depth_start.push_back((int)s->shared_top.size());
    if (all)
    {
        s->shared_mesh_tri_base.assign(s->mesh_bounds.size() / 6, 0u);   // per mesh, once: its first triangle in the concatenated attribute arrays
        for (size_t i = I; i-- > 0;) s->shared_mesh_tri_base[s->inst_mesh[i]] = s->inst_host[i].mesh_tri_base;
        HR_HIP(hipMemcpyAsync(s->dev_inst_mesh.p, s->inst_mesh.data(), I * 4, hipMemcpyHostToDevice, st));
        return shared_device_mesh_table_upload(s, st);
    }
    return HR_OK;
}

namespace {
// the one wait of a read-back: the stream of the last device update — or the device, once an update has been captured (its replays run on
// streams this library never sees)
hr_status wait_for_device_update(const hr_scene* s)
{
    HR_HIP(hipSetDevice(s->ctx->device));
    if (s->masks_captured || (s->masks_on_device && !s->dev_update)) HR_HIP(hipDeviceSynchronize());
    else
    {
        if (s->masks_on_device) HR_HIP(hipStreamSynchronize(s->mask_stream));   // hr_scene_set_instance_masks_device: the records it wrote
        if (s->dev_update && !s->dev_update->captured) HR_HIP(hipStreamSynchronize(s->dev_update->last_stream));
        else HR_HIP(hipDeviceSynchronize());
    }
    return HR_OK;
}
} // namespace

hr_status hr::shared_device_status_refresh(const hr_scene* s)
{
    SharedDeviceUpdate& du = *s->dev_update;
    if (du.status_stale || du.captured)
    {
        const hr_status w = wait_for_device_update(s);
        if (w != HR_OK) return w;
        HR_HIP(hipMemcpy(du.status_host, du.status.p, sizeof(DeviceUpdateStatus), hipMemcpyDeviceToHost));
        du.status_stale = false;
    }
    return HR_OK;
}

hr_status hr::shared_mirrors_refresh(hr_scene* s)
{
    if (!s->mirrors_stale) return HR_OK;
    const size_t I = (size_t)s->n_instances;
    {
        const hr_status w = wait_for_device_update(s);
        if (w != HR_OK) return w;
    }
    s->shared_host.resize(I);
    HR_HIP(hipMemcpy(s->shared_host.data(), s->inst_shared.p, I * sizeof(InstanceShared), hipMemcpyDeviceToHost));
    if (s->fixed_shape)   // a device re-build decides the order of the leaves where the host cannot see it
    {
        HR_HIP(hipMemcpy(s->shared_leaf_inst.data(), s->dev_leaf_inst.p, I * 4, hipMemcpyDeviceToHost));
        HR_HIP(hipMemcpy(s->shared_leaf_of.data(), s->dev_leaf_of.p, I * 4, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < I; i++)
    {
        const InstanceShared& r = s->shared_host[(size_t)s->shared_leaf_of[i]];
        std::memcpy(s->inst_host[i].m, r.m, 64);
        s->inst_mask[i] = (uint8_t)((r.flags & kInstanceMaskBits) >> kInstanceMaskShift);   // hr_scene_set_instance_masks_device wrote them unseen
    }
    s->masks_on_device = false;
    s->mirrors_stale = (s->dev_update && s->dev_update->captured) || s->masks_captured;   // sticky: a replay may rewrite the records at any time
    if (s->dev_update) s->dev_update->stream_waits++;
    return HR_OK;
}

extern "C" {

hr_status hr_scene_update_instances_device(hr_scene* scene, const float* model_matrices, const float* world_bounds, void* stream)
{
    try
    {
        return update_device_impl(scene, model_matrices, world_bounds, (hipStream_t)stream);
    }
    catch (const std::bad_alloc&)
    {
        set_last_error("hr_scene_update_instances_device: host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

hr_status hr_scene_device_update_status(const hr_scene* scene, float* top_cost_ratio, int32_t* rejected_instances, int32_t* bounds_violated)
{
    static const char* call = "hr_scene_device_update_status";
    if (!scene) return bad(call, "scene is NULL");
    if (!scene->shared) return bad(call, "not a shared instanced scene (hr_scene_create_instanced_shared)");
    float ratio = 1.0f;
    int32_t rej = 0, vio = 0;
    if (scene->dev_update)
    {
        SharedDeviceUpdate& du = *scene->dev_update;
        const hr_status w = shared_device_status_refresh(scene);
        if (w != HR_OK) return w;
        const DeviceUpdateStatus* hs = (const DeviceUpdateStatus*)du.status_host;
        // after a device re-build the ratio is relative to the re-built top level's sum, not to the last host build's
        const double base = du.device_baseline ? hs->baseline : du.area_at_build;
        if (base > 0.0) ratio = (float)(hs->area / base);
        rej = (int32_t)hs->rejected; vio = du.given_bounds ? (int32_t)hs->violated : 0;
    }
    if (top_cost_ratio) *top_cost_ratio = ratio;
    if (rejected_instances) *rejected_instances = rej;
    if (bounds_violated) *bounds_violated = vio;
    return HR_OK;
}

hr_status hr_scene_device_update_stats(const hr_scene* scene, int64_t* launches, int64_t* stream_waits)
{
    static const char* call = "hr_scene_device_update_stats";
    if (!scene) return bad(call, "scene is NULL");
    if (!scene->shared) return bad(call, "not a shared instanced scene (hr_scene_create_instanced_shared)");
    if (launches) *launches = scene->dev_update ? scene->dev_update->launches : 0;
    if (stream_waits) *stream_waits = scene->dev_update ? scene->dev_update->stream_waits : 0;
    return HR_OK;
}

} // extern "C"
