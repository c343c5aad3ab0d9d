// Alpha-tested cutout materials: the host side (the accept test itself is cutout.h cutout_accept, called by every walk).
//
// hr_scene_set_alpha_cutoffs copies its argument into pinned staging the scene owns (the next call waits for the copy's event before it rewrites
// the staging), copies that to the device on `stream` and ends in ONE kernel, k_cutout_table, which derives the per-attribute-index table the walks
// read from tri_material, the cutoffs and the materials' albedo textures.  The table is keyed on what `prim` already names — never on a word of
// TriGPU — so refits, deforms, instance updates and every kind of re-build leave it alone.  Allocates at the first call that sets a cutoff above 0; the arguments are checked against host state alone, before the device is touched.
// The cutoffs' host copy and the per-class opaque flags are host state, read when a pass or query enqueues its launch.
#include "cutout_host.h"
#include "instances_shared_device.h"
#include <cmath>
#include <cstring>

using namespace hr;

namespace {

__global__ void __launch_bounds__(256) k_cutout_table(uint2* tab, const uint32_t* tri_material, const float* cutoffs, const int32_t* mat_tex, int n_materials, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = tri_material ? tri_material[i] : 0u;
    uint2 e = make_uint2(0u, 0u);
    if (m < (uint32_t)n_materials)   // creation checked every index; the guard keeps a damaged array in bounds
    {
        const float   c   = cutoffs[m];
        const int32_t tex = mat_tex[(size_t)m * 6];
        if (c > 0.0f && tex >= 0) e = make_uint2((uint32_t)tex + 1u, __float_as_uint(c));
    }
    tab[i] = e;
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

// every call of this file: a flat, deformable or shared scene; a private-copy instanced scene refuses
hr_status scene_check(const hr_scene* s, const char* call)
{
    if (!s) return bad(call, "scene is NULL");
    if (s->n_instances > 0 && !s->shared)
    {
        set_last_error(std::string(call) + ": a private-copy instanced scene (hr_scene_create_instanced) has no cutout materials; use hr_scene_create_instanced_shared");
        return HR_ERR_UNSUPPORTED;
    }
    return HR_OK;
}

size_t attribute_triangles(const hr_scene* s) { return s->shared ? s->mesh_positions.bytes / 36 : (size_t)s->info.n_tris; }

hr_status set_cutoffs(hr_scene* s, const float* cutoffs, hipStream_t st)
{
    static const char* call = "hr_scene_set_alpha_cutoffs";
    hr_status e = scene_check(s, call);
    if (e != HR_OK) return e;
    if (!cutoffs) return bad(call, "cutoffs is NULL");
    const size_t M = (size_t)s->n_materials;
    bool any = false;
    for (size_t m = 0; m < M; m++)
    {
        if (!std::isfinite(cutoffs[m])) return bad(call, "cutoffs[" + std::to_string(m) + "] is not finite");
        any = any || cutoffs[m] > 0.0f;
    }
    if (any)
    {
        if (!s->has_textures) return bad(call, "a cutoff above 0 in a scene without textures");
        if (!s->has_uvs) return bad(call, "a cutoff above 0 in a scene without uvs");
        for (size_t m = 0; m < M; m++)
            if (cutoffs[m] > 0.0f && (m >= s->mat_albedo_host.size() || s->mat_albedo_host[m] < 0))
                return bad(call, "cutoffs[" + std::to_string(m) + "] is above 0 and material " + std::to_string(m) + " has no albedo texture");
    }
    if (!any && !s->cutoff_stage)   // nothing was ever enabled: no table exists and none is needed
    {
        s->alpha_cutoffs.assign(cutoffs, cutoffs + M);
        return HR_OK;
    }
    // every argument is accepted: from here on only the device can fail
    HR_HIP(hipSetDevice(s->ctx->device));
    if (stream_is_capturing(st)) return bad(call, "stages through memory the next call rewrites: not possible while the stream is capturing");
    const size_t n = attribute_triangles(s);
    if (!s->cutoff_stage)
    {
        // all four or none: cutoff_stage, set last, is what says "allocated"
        float*     stage = nullptr;
        hipEvent_t done = nullptr;
        e = s->cutoff_dev.alloc(M * 4);
        if (e == HR_OK) e = s->cutout_tab.alloc(n * 8);
        if (e == HR_OK && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) { done = nullptr; set_last_error(std::string(call) + ": hipEventCreateWithFlags failed"); e = HR_ERR_HIP; }
        if (e == HR_OK && hipHostMalloc((void**)&stage, M * 4, hipHostMallocDefault) != hipSuccess) { stage = nullptr; set_last_error(std::string(call) + ": hipHostMalloc failed"); e = HR_ERR_OUT_OF_MEMORY; }
        if (e != HR_OK)
        {
            (void)hipGetLastError();
            if (done) (void)hipEventDestroy(done);
            s->cutoff_dev.free(); s->cutout_tab.free();
            return e;
        }
        s->cutoff_copied = done;
        s->cutoff_stage = stage;
    }
    else
        HR_HIP(hipEventSynchronize(s->cutoff_copied));   // the staging may still feed the previous call's copy
    std::memcpy(s->cutoff_stage, cutoffs, M * 4);
    HR_HIP(hipMemcpyAsync(s->cutoff_dev.p, s->cutoff_stage, M * 4, hipMemcpyHostToDevice, st));
    HR_HIP(hipEventRecord(s->cutoff_copied, st));
    if (n > 0)
    {
        const uint32_t* tri_material = s->has_material ? (const uint32_t*)(s->shared ? s->mesh_material.p : s->tri_material.p) : nullptr;
        hipLaunchKernelGGL(k_cutout_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint2*)s->cutout_tab.p, tri_material, (const float*)s->cutoff_dev.p,
                           (const int32_t*)s->mat_tex.p, (int)M, (long long)n);
        HR_HIP(hipGetLastError());
    }
    s->alpha_cutoffs.assign(cutoffs, cutoffs + M);
    s->cutout_enabled = any;
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

bool hr::reject_cutout_dev_switches(const hr_scene* s, int ray_class, const char* call, bool wanted)
{
    if (!wanted || !cutout_on(s, ray_class)) return false;
    set_last_error(std::string(call) + ": trace statistics and developer switches are not available while the scene's alpha cutoffs are enabled (hr_scene_set_alpha_cutoffs)");
    return true;
}

extern "C" {

hr_status hr_scene_set_alpha_cutoffs(hr_scene* scene, const float* cutoffs, void* stream)
{
    return no_throw("hr_scene_set_alpha_cutoffs", [&] { return set_cutoffs(scene, cutoffs, (hipStream_t)stream); });
}

hr_status hr_scene_get_alpha_cutoffs(const hr_scene* scene, float* cutoffs_out)
{
    static const char* call = "hr_scene_get_alpha_cutoffs";
    const hr_status e = scene_check(scene, call);
    if (e != HR_OK) return e;
    if (!cutoffs_out) return bad(call, "cutoffs_out is NULL");
    for (size_t m = 0; m < (size_t)scene->n_materials; m++) cutoffs_out[m] = scene->alpha_cutoffs.empty() ? 0.0f : scene->alpha_cutoffs[m];
    return HR_OK;
}

hr_status hr_scene_set_ray_class_opaque(hr_scene* scene, int32_t ray_class, int32_t force_opaque)
{
    static const char* call = "hr_scene_set_ray_class_opaque";
    const hr_status e = scene_check(scene, call);
    if (e != HR_OK) return e;
    if (ray_class < 0 || ray_class >= HR_RAY_CLASS_COUNT) return bad(call, "ray_class " + std::to_string(ray_class) + " is outside [0, HR_RAY_CLASS_COUNT)");
    scene->class_opaque[ray_class] = force_opaque != 0 ? 1 : 0;
    return HR_OK;
}

hr_status hr_scene_get_ray_class_opaque(const hr_scene* scene, int32_t ray_class, int32_t* force_opaque)
{
    static const char* call = "hr_scene_get_ray_class_opaque";
    const hr_status e = scene_check(scene, call);
    if (e != HR_OK) return e;
    if (ray_class < 0 || ray_class >= HR_RAY_CLASS_COUNT) return bad(call, "ray_class " + std::to_string(ray_class) + " is outside [0, HR_RAY_CLASS_COUNT)");
    if (!force_opaque) return bad(call, "force_opaque is NULL");
    *force_opaque = scene->class_opaque[ray_class];
    return HR_OK;
}

} // extern "C"
