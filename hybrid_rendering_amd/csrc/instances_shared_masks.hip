// Instance masks and per-ray-class cull masks of a shared instanced scene (instances_shared.hip): Vulkan's rule — a ray walks into an instance
// iff (instance mask & the ray's cull mask) != 0 (VkAccelerationStructureInstanceKHR::mask against the cull mask of rayQueryInitializeEXT /
// traceRayEXT, which the reference passes in every ray it fires).  A rejected instance does not exist for the ray (traverse2.h enter_instance).
//
// The instance mask lives in bits 8..15 of InstanceShared::flags (bvh.h), in the quad the walk holds at an instance's entry anyway.  Both setters end
// in ONE kernel, k_set_masks, which scatters a byte per instance into the records through dev_leaf_of — the device's own instance -> leaf table, so a
// device re-build of the top level (which re-orders the leaves where the host cannot see it) needs no care.  Every other writer of a record keeps the
// bits: fill_record takes them from hr_scene::inst_mask, k_shared_records masks them in, k_gather / k_commit move whole records.
//   hr_scene_set_instance_masks          copies its argument into pinned staging (guarded by the scene's upload fence: the next call waits before it
//                                        rewrites it), one copy to the device, the kernel.  Allocates at the first call.
//   hr_scene_set_instance_masks_device   the kernel alone: no allocation, no wait, legal under stream capture.  The host's knowledge of the masks is
//                                        stale from then on (mirrors_stale): the next host call reads the records back, as after a device update.
// No box changes, so geometry_epoch stays and AO's entry table with it.
// The cull masks are host state (hr_scene::cull_mask), read when a pass or query enqueues its launch and passed in the kernel arguments.
#include "instances_shared_device.h"
#include <cstring>

using namespace hr;

namespace {

__global__ void __launch_bounds__(256) k_set_masks(InstanceShared* records, const int32_t* leaf_of, const uint8_t* masks, int n)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int32_t leaf = leaf_of[i];
    if ((uint32_t)leaf >= (uint32_t)n) return;   // a table that is always a permutation; the guard keeps a damaged one in bounds
    uint32_t& f = records[leaf].flags;
    f = (f & ~kInstanceMaskBits) | ((uint32_t)masks[i] << kInstanceMaskShift);
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

// every call of this file: a shared scene or HR_ERR_INVALID_ARG, before anything else happens
hr_status scene_check(const hr_scene* s, const char* call)
{
    if (!s) return bad(call, "scene is NULL");
    if (!s->shared)
        return bad(call, "not a shared instanced scene (hr_scene_create_instanced_shared): the single-level walk of flat and private-copy scenes has no instance boundary to reject at");
    return HR_OK;
}

hr_status enqueue(hr_scene* s, const uint8_t* dev_masks, hipStream_t st)
{
    const int I = s->n_instances;
    hipLaunchKernelGGL(k_set_masks, dim3(cdiv(I, 256)), dim3(256), 0, st, (InstanceShared*)s->inst_shared.p, (const int32_t*)s->dev_leaf_of.p, dev_masks, I);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status set_host(hr_scene* s, const uint8_t* masks, hipStream_t st)
{
    static const char* call = "hr_scene_set_instance_masks";
    hr_status e = scene_check(s, call);
    if (e != HR_OK) return e;
    if (!masks) return bad(call, "masks is NULL");
    HR_HIP(hipSetDevice(s->ctx->device));
    if (stream_is_capturing(st)) return bad(call, "the host form stages through memory the next call rewrites: not possible while the stream is capturing (use hr_scene_set_instance_masks_device)");
    const size_t I = (size_t)s->n_instances;
    if (!s->mask_stage)
    {
        if ((e = s->mask_dev.alloc(I)) != HR_OK) return e;
        HR_HIP(hipHostMalloc((void**)&s->mask_stage, I ? I : 1, hipHostMallocDefault));
    }
    if ((e = instanced_scene_wait_uploads(s)) != HR_OK) return e;   // the staging may still feed the previous call's copy
    std::memcpy(s->mask_stage, masks, I);
    HR_HIP(hipMemcpyAsync(s->mask_dev.p, s->mask_stage, I, hipMemcpyHostToDevice, st));
    if ((e = enqueue(s, (const uint8_t*)s->mask_dev.p, st)) != HR_OK) return e;
    if ((e = instanced_scene_mark_uploads(s, st)) != HR_OK) return e;
    // every mask is rewritten, so nothing has to be read back for this; what the host knows is what it has just been told — until a captured
    // device call replays (masks_captured keeps mirrors_stale set)
    s->inst_mask.assign(masks, masks + I);
    return HR_OK;
}

hr_status set_device(hr_scene* s, const uint8_t* masks, hipStream_t st)
{
    static const char* call = "hr_scene_set_instance_masks_device";
    const hr_status e = scene_check(s, call);
    if (e != HR_OK) return e;
    if (!masks) return bad(call, "masks is NULL");
    HR_HIP(hipSetDevice(s->ctx->device));
    const bool capturing = stream_is_capturing(st);
    const hr_status q = enqueue(s, masks, st);
    if (q != HR_OK) return q;
    s->mask_stream = st;
    s->masks_on_device = true;
    s->masks_captured = s->masks_captured || capturing;   // replays run it unseen: the mirrors count as stale before every host call from now on
    s->mirrors_stale = true;
    return HR_OK;
}

hr_status get_host(const hr_scene* s, uint8_t* out)
{
    static const char* call = "hr_scene_get_instance_masks";
    const hr_status e = scene_check(s, call);
    if (e != HR_OK) return e;
    if (!out) return bad(call, "masks_out is NULL");
    if (s->mirrors_stale)
    {
        HR_HIP(hipSetDevice(s->ctx->device));
        const hr_status ws = instanced_scene_wait_uploads(const_cast<hr_scene*>(s));   // the read-back rewrites the host tail's staging
        if (ws != HR_OK) return ws;
        const hr_status ms = shared_mirrors_refresh(const_cast<hr_scene*>(s));
        if (ms != HR_OK) return ms;
    }
    std::memcpy(out, s->inst_mask.data(), (size_t)s->n_instances);
    return HR_OK;
}

template <class F>
hr_status no_throw(const char* call, F f)
{
    try { return f(); }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

} // namespace

extern "C" {

hr_status hr_scene_set_instance_masks(hr_scene* scene, const uint8_t* masks, void* stream)
{
    return no_throw("hr_scene_set_instance_masks", [&] { return set_host(scene, masks, (hipStream_t)stream); });
}

hr_status hr_scene_set_instance_masks_device(hr_scene* scene, const uint8_t* masks, void* stream)
{
    return no_throw("hr_scene_set_instance_masks_device", [&] { return set_device(scene, masks, (hipStream_t)stream); });
}

hr_status hr_scene_get_instance_masks(const hr_scene* scene, uint8_t* masks_out)
{
    return no_throw("hr_scene_get_instance_masks", [&] { return get_host(scene, masks_out); });
}

hr_status hr_scene_set_cull_mask(hr_scene* scene, int32_t ray_class, uint32_t mask)
{
    static const char* call = "hr_scene_set_cull_mask";
    const hr_status e = scene_check(scene, call);
    if (e != HR_OK) return e;
    if (ray_class < 0 || ray_class >= HR_RAY_CLASS_COUNT) return bad(call, "ray_class " + std::to_string(ray_class) + " is outside [0, HR_RAY_CLASS_COUNT)");
    if (mask > 0xFFu) return bad(call, "mask " + std::to_string(mask) + " is above 0xFF");
    scene->cull_mask[ray_class] = mask;
    return HR_OK;
}

hr_status hr_scene_get_cull_mask(const hr_scene* scene, int32_t ray_class, uint32_t* mask)
{
    static const char* call = "hr_scene_get_cull_mask";
    const hr_status e = scene_check(scene, call);
    if (e != HR_OK) return e;
    if (ray_class < 0 || ray_class >= HR_RAY_CLASS_COUNT) return bad(call, "ray_class " + std::to_string(ray_class) + " is outside [0, HR_RAY_CLASS_COUNT)");
    if (!mask) return bad(call, "mask is NULL");
    *mask = scene->cull_mask[ray_class];
    return HR_OK;
}

} // extern "C"
