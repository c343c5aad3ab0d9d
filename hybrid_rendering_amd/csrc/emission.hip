// Emissive materials: the host side, the raw query, the emissive image of the primary hits and the add stage after the composite
// (contract: include/hr_emission.h; DESIGN.md §7 "Emissive materials"; the emission function itself is emission.h, called by the EMISSIVE trace instantiations too).
//
// The setters follow hr_scene_set_alpha_cutoffs (cutout.hip): host state read when a pass or query enqueues, per-material device tables allocated by
// the first setter call, the host forms staged through pinned memory the scene owns (the next call waits for the copy's event before it rewrites
// the staging).  The arguments are checked against host state alone, before the device is touched.
#include "emission_host.h"
#include "cutout_host.h"
#include "instances_shared_device.h"
#include "pixel_dir.h"
#include "../../include/hr_emission.h"
#include <cmath>
#include <cstring>

using namespace hr;

namespace {

// ---- hr_scene_emission ---------------------------------------------------------------------------------------------------------------------
// inst: instanced kinds, per instance { first_tri, mesh_tri_base } in the scene desc's order, then { total triangles, 0 }; null for a flat scene,
// whose attribute index is the triangle.  The numbering is hr_trace_closest_hit's on every kind.
__global__ void __launch_bounds__(256) k_emission_query(EmissionView em, SceneShading sh, const uint2* inst, int n_instances, long long n_tris, long long n,
                                                         const int32_t* prim, const float* tuv, float* out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    f3 E = mk3(0.0f, 0.0f, 0.0f);
    const int32_t p = prim[i];
    if (p >= 0 && (long long)p < n_tris)
    {
        size_t q = (size_t)p;
        if (inst)
        {
            int lo = 0, hi = n_instances;   // the last instance whose first_tri <= p
            while (hi - lo > 1)
            {
                const int mid = (lo + hi) >> 1;
                if (inst[mid].x <= (uint32_t)p) lo = mid; else hi = mid;
            }
            q = (size_t)inst[lo].y + ((uint32_t)p - inst[lo].x);
        }
        f3 e;
        if (emission_at(em, sh, q, tuv[i * 3 + 1], tuv[i * 3 + 2], e)) E = e;
    }
    out[i * 3 + 0] = E.x; out[i * 3 + 1] = E.y; out[i * 3 + 2] = E.z;
}

// ---- hr_gbuffer_emissive -------------------------------------------------------------------------------------------------------------------
struct EmissiveImageArgs
{
    float         vpi[16];
    float         cam[3];
    int           w, h;
    const Node8*  nodes;
    const TriGPU* tris;
    SceneShading  sh;
    uint2*        out;
};

// k_gbuffer_raycast's tiling, ray and walk (api.hip), then E instead of the G-buffer's texel
template <bool TWO_LEVEL, bool CUTOUT>
__global__ __launch_bounds__(256) void k_gbuffer_emissive(EmissiveImageArgs a, EmissionView em, CutoutView cv)
{
    __shared__ uint32_t s_stack[4][HR_STACK_ENTRIES * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles_x = (a.w + 7) / 8, tiles_y = (a.h + 7) / 8;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= tiles_x * tiles_y) return;
    const int x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3);
    if (x >= a.w || y >= a.h) return;
    const size_t i   = (size_t)y * a.w + x;
    const f3     cam = mk3(a.cam[0], a.cam[1], a.cam[2]);
    const f3     d   = gb_pixel_dir(a, (float)x + 0.5f, (float)y + 0.5f);
    const HitOf<TWO_LEVEL> hit = trace_closest_of<TWO_LEVEL, CUTOUT>(a.nodes, a.tris, a.sh.inst_shared, a.sh.cull[HR_RAY_PRIMARY], cam, d, 0.0f, 1.0e30f, s_stack[wave], lane, cv);
    if (hit.prim < 0) { a.out[i] = make_uint2(0u, 0u); return; }
    f3 E = mk3(0.0f, 0.0f, 0.0f), e;
    if (emission_at_hit(em, a.sh, hit, e)) E = e;
    a.out[i] = make_uint2(pack_h2(E.x, E.y), pack_h2(E.z, 1.0f));
}

// ---- hr_deferred_add_emissive --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_add_emissive(uint2* colour, const uint2* emissive, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 c = colour[i], e = emissive[i];
    colour[i] = make_uint2(pack_h2(h2f_lo(c.x) + h2f_lo(e.x), h2f_hi(c.x) + h2f_hi(e.x)), (c.y & 0xffff0000u) | (pack_h2(h2f_lo(c.y) + h2f_lo(e.y), 0.0f) & 0xffffu));
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

int n_textures_of(const hr_scene* s) { return s->has_textures ? (int)(s->tex_table.bytes / 16) : 0; }

// what the host knows: does some material emit?
void refresh_any(hr_scene* s)
{
    bool any = s->emissive_on_device;
    for (float v : s->emissive_host) any = any || v != 0.0f;
    for (int32_t t : s->emissive_tex_host) any = any || t >= 0;
    s->emission_any = any;
}

// the first setter call: the tables (never empty: a scene without materials gets one row that emission_at, which returns false for a material index
// at or above n_materials, never reads), filled from the description's constants and "no texture", the pinned staging and its event.  All or none: em_stage, set last, is what says "allocated".  Synchronous, like creation.
hr_status ensure_tables(hr_scene* s, const char* call, hipStream_t st)
{
    if (s->em_stage) return HR_OK;
    HR_HIP(hipSetDevice(s->ctx->device));
    if (stream_is_capturing(st)) return bad(call, "the first call allocates: not possible while the stream is capturing");
    const size_t M = (size_t)s->n_materials, rows = M ? M : 1;
    std::vector<float>   mats(M * 8), rgb(rows * 3, 0.0f);
    std::vector<int32_t> tex(rows, -1);
    if (M) HR_HIP(hipMemcpy(mats.data(), s->materials.p, M * 32, hipMemcpyDeviceToHost));
    for (size_t m = 0; m < M; m++)
        for (int c = 0; c < 3; c++) rgb[m * 3 + c] = mats[m * 8 + 5 + c];
    float*     stage = nullptr;
    hipEvent_t done = nullptr;
    hr_status  e = s->em_rgb.alloc(rows * 12);
    if (e == HR_OK) e = s->em_tex.alloc(rows * 4);
    if (e == HR_OK && hipMemcpy(s->em_rgb.p, rgb.data(), rows * 12, hipMemcpyHostToDevice) != hipSuccess) { set_last_error(std::string(call) + ": hipMemcpy failed"); e = HR_ERR_HIP; }
    if (e == HR_OK && hipMemcpy(s->em_tex.p, tex.data(), rows * 4, hipMemcpyHostToDevice) != hipSuccess) { set_last_error(std::string(call) + ": hipMemcpy failed"); e = HR_ERR_HIP; }
    if (e == HR_OK && s->n_instances > 0)
    {
        // hr_scene_emission's map from hr_trace_closest_hit's triangle numbers to attribute indices; the fields never change after creation
        std::vector<uint2> tab((size_t)s->n_instances + 1);
        uint64_t total = 0;
        for (int i = 0; i < s->n_instances; i++)
        {
            const InstanceRec& r = s->inst_host[(size_t)i];
            tab[(size_t)i] = make_uint2(r.first_tri, r.mesh_tri_base);
            total = (uint64_t)r.first_tri + r.n_tris;
        }
        tab[(size_t)s->n_instances] = make_uint2((uint32_t)total, 0u);
        e = s->em_inst.alloc(tab.size() * 8);
        if (e == HR_OK && hipMemcpy(s->em_inst.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { set_last_error(std::string(call) + ": hipMemcpy failed"); e = HR_ERR_HIP; }
    }
    if (e == HR_OK && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) { done = nullptr; set_last_error(std::string(call) + ": hipEventCreateWithFlags failed"); e = HR_ERR_HIP; }
    if (e == HR_OK && hipHostMalloc((void**)&stage, rows * 16, hipHostMallocDefault) != hipSuccess) { stage = nullptr; set_last_error(std::string(call) + ": hipHostMalloc failed"); e = HR_ERR_OUT_OF_MEMORY; }
    if (e != HR_OK)
    {
        (void)hipGetLastError();
        if (done) (void)hipEventDestroy(done);
        s->em_rgb.free(); s->em_tex.free(); s->em_inst.free();
        return e;
    }
    rgb.resize(M * 3); tex.resize(M);
    s->emissive_host = rgb; s->emissive_tex_host = tex;
    s->em_copied = done;
    s->em_stage = stage;
    refresh_any(s);
    return HR_OK;
}

// -1: every component the host knows is finite and >= 0
long long first_bad_constant(const float* rgb, size_t M)
{
    for (size_t k = 0; k < M * 3; k++)
        if (!std::isfinite(rgb[k]) || rgb[k] < 0.0f) return (long long)(k / 3);
    return -1;
}

hr_status set_emission(hr_scene* s, int32_t enable, float scale, hipStream_t st)
{
    static const char* call = "hr_scene_set_emission";
    if (!s) return bad(call, "scene is NULL");
    if (!(std::isfinite(scale) && scale >= 0.0f)) return bad(call, "scale is not a finite number >= 0");
    if (!enable && !s->em_stage) { s->emission_enabled = false; s->emission_scale = scale; return HR_OK; }   // nothing was ever set: no table is needed
    const hr_status e = ensure_tables(s, call, st);
    if (e != HR_OK) return e;
    if (enable && !s->emissive_on_device)
    {
        const long long m = first_bad_constant(s->emissive_host.data(), (size_t)s->n_materials);
        if (m >= 0) return bad(call, "material " + std::to_string(m) + " has an emissive component that is not finite or is negative");
    }
    s->emission_enabled = enable != 0;
    s->emission_scale = scale;
    return HR_OK;
}

// the host forms: both rows of the staging go to the device again (a few bytes per material)
hr_status upload_host_tables(hr_scene* s, const char* call, const float* rgb, const int32_t* tex, hipStream_t st)
{
    if (stream_is_capturing(st)) return bad(call, "stages through memory the next call rewrites: not possible while the stream is capturing");
    const size_t M = (size_t)s->n_materials;
    if (M == 0) return HR_OK;
    HR_HIP(hipEventSynchronize(s->em_copied));   // the staging may still feed the previous call's copy
    int32_t* stage_tex = (int32_t*)(s->em_stage + M * 3);
    if (rgb)
    {
        std::memcpy(s->em_stage, rgb, M * 12);
        HR_HIP(hipMemcpyAsync(s->em_rgb.p, s->em_stage, M * 12, hipMemcpyHostToDevice, st));
    }
    if (tex)
    {
        std::memcpy(stage_tex, tex, M * 4);
        HR_HIP(hipMemcpyAsync(s->em_tex.p, stage_tex, M * 4, hipMemcpyHostToDevice, st));
    }
    HR_HIP(hipEventRecord(s->em_copied, st));
    return HR_OK;
}

hr_status set_emissive(hr_scene* s, const float* rgb, hipStream_t st)
{
    static const char* call = "hr_scene_set_emissive";
    if (!s) return bad(call, "scene is NULL");
    if (!rgb) return bad(call, "rgb is NULL");
    const long long m = first_bad_constant(rgb, (size_t)s->n_materials);
    if (m >= 0) return bad(call, "rgb[" + std::to_string(m) + "] has a component that is not finite or is negative");
    hr_status e = ensure_tables(s, call, st);
    if (e != HR_OK) return e;
    if ((e = upload_host_tables(s, call, rgb, nullptr, st)) != HR_OK) return e;
    s->emissive_host.assign(rgb, rgb + (size_t)s->n_materials * 3);
    s->emissive_on_device = false;
    refresh_any(s);
    return HR_OK;
}

hr_status set_emissive_device(hr_scene* s, const float* rgb, hipStream_t st)
{
    static const char* call = "hr_scene_set_emissive_device";
    if (!s) return bad(call, "scene is NULL");
    if (!rgb) return bad(call, "rgb is NULL");
    const hr_status e = ensure_tables(s, call, st);
    if (e != HR_OK) return e;
    if (s->n_materials > 0) HR_HIP(hipMemcpyAsync(s->em_rgb.p, rgb, (size_t)s->n_materials * 12, hipMemcpyDeviceToDevice, st));
    s->emissive_on_device = true;
    refresh_any(s);
    return HR_OK;
}

hr_status set_emissive_textures(hr_scene* s, const int32_t* tex, hipStream_t st)
{
    static const char* call = "hr_scene_set_emissive_textures";
    if (!s) return bad(call, "scene is NULL");
    if (!tex) return bad(call, "tex is NULL");
    const int T = n_textures_of(s);
    for (int m = 0; m < s->n_materials; m++)
    {
        if (tex[m] < -1) return bad(call, "tex[" + std::to_string(m) + "] is below -1");
        if (tex[m] >= 0 && T == 0) return bad(call, "tex[" + std::to_string(m) + "] names a texture and the scene has none");
        if (tex[m] >= T && tex[m] >= 0) return bad(call, "tex[" + std::to_string(m) + "] = " + std::to_string(tex[m]) + " is outside the scene's " + std::to_string(T) + " textures");
    }
    hr_status e = ensure_tables(s, call, st);
    if (e != HR_OK) return e;
    if ((e = upload_host_tables(s, call, nullptr, tex, st)) != HR_OK) return e;
    s->emissive_tex_host.assign(tex, tex + (size_t)s->n_materials);
    refresh_any(s);
    return HR_OK;
}

// a view for a scene whose tables may not exist yet: without them nothing emits
EmissionView view_or_dark(const hr_scene* s)
{
    EmissionView em = emission_view_of(s);
    if (!s->em_stage) em.n_materials = 0;
    return em;
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

bool hr::reject_emission_dev_switches(const hr_scene* s, const char* call, bool wanted)
{
    if (!wanted || !emission_live(s)) return false;
    set_last_error(std::string(call) + ": trace statistics and developer switches are not available while the scene's emission is enabled (hr_scene_set_emission)");
    return true;
}

extern "C" {

hr_status hr_scene_set_emission(hr_scene* scene, int32_t enable, float scale, void* stream)
{
    return no_throw("hr_scene_set_emission", [&] { return set_emission(scene, enable, scale, (hipStream_t)stream); });
}

hr_status hr_scene_get_emission(const hr_scene* scene, int32_t* enable, float* scale)
{
    static const char* call = "hr_scene_get_emission";
    if (!scene) return bad(call, "scene is NULL");
    if (!enable && !scale) return bad(call, "enable and scale are both NULL");
    if (enable) *enable = scene->emission_enabled ? 1 : 0;
    if (scale) *scale = scene->emission_scale;
    return HR_OK;
}

hr_status hr_scene_set_emissive(hr_scene* scene, const float* rgb, void* stream)
{
    return no_throw("hr_scene_set_emissive", [&] { return set_emissive(scene, rgb, (hipStream_t)stream); });
}

hr_status hr_scene_set_emissive_device(hr_scene* scene, const float* rgb, void* stream)
{
    return no_throw("hr_scene_set_emissive_device", [&] { return set_emissive_device(scene, rgb, (hipStream_t)stream); });
}

hr_status hr_scene_set_emissive_textures(hr_scene* scene, const int32_t* tex, void* stream)
{
    return no_throw("hr_scene_set_emissive_textures", [&] { return set_emissive_textures(scene, tex, (hipStream_t)stream); });
}

hr_status hr_scene_emission(const hr_scene* scene, int64_t n, const int32_t* prim, const float* tuv, float* out, void* stream)
{
    static const char* call = "hr_scene_emission";
    if (!scene) return bad(call, "scene is NULL");
    if (n < 0) return bad(call, "n is negative");
    if (n == 0) return HR_OK;
    if (!prim) return bad(call, "prim is NULL");
    if (!tuv) return bad(call, "tuv is NULL");
    if (!out) return bad(call, "out is NULL");
    HR_HIP(hipSetDevice(scene->ctx->device));
    SceneShading sh;
    scene_shading_from(scene, sh);
    const EmissionView em = view_or_dark(scene);
    // before the first setter call the instance map does not exist, and nothing emits: the kernel never reads it
    const uint2* inst = scene->n_instances > 0 && scene->em_stage ? (const uint2*)scene->em_inst.p : nullptr;
    long long n_tris = scene->n_instances > 0 ? 0 : (long long)scene->info.n_tris;
    if (scene->n_instances > 0 && !scene->inst_host.empty()) n_tris = (long long)scene->inst_host.back().first_tri + scene->inst_host.back().n_tris;
    if (scene->n_instances > 0 && !inst) n_tris = 0;
    hipLaunchKernelGGL(k_emission_query, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, em, sh, inst, scene->n_instances, n_tris, (long long)n, prim, tuv, out);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_gbuffer_emissive(const hr_scene* scene, const hr_ubo* ubo, int32_t width, int32_t height, void* out, void* stream)
{
    static const char* call = "hr_gbuffer_emissive";
    if (!scene) return bad(call, "scene is NULL");
    if (!ubo) return bad(call, "ubo is NULL");
    if (width <= 0 || height <= 0) return bad(call, "width or height is not positive");
    if (!out) return bad(call, "out is NULL");
    HR_HIP(hipSetDevice(scene->ctx->device));
    EmissiveImageArgs a;
    for (int i = 0; i < 16; i++) a.vpi[i] = ubo->view_proj_inverse[i];
    for (int i = 0; i < 3; i++) a.cam[i] = ubo->cam_pos[i];
    a.w = width; a.h = height;
    a.nodes = (const Node8*)scene->nodes.p; a.tris = (const TriGPU*)scene->tris.p;
    scene_shading_from(scene, a.sh);
    a.out = (uint2*)out;
    const bool       cutout = cutout_on(scene, HR_RAY_PRIMARY);
    const CutoutView cv = cutout ? cutout_view_of(scene) : CutoutView();
    void (*const kernel[2][2])(EmissiveImageArgs, EmissionView, CutoutView) = { { k_gbuffer_emissive<false, false>, k_gbuffer_emissive<false, true> },
                                                                                { k_gbuffer_emissive<true, false>, k_gbuffer_emissive<true, true> } };
    const int tiles = ((width + 7) / 8) * ((height + 7) / 8);
    hipLaunchKernelGGL(kernel[scene->shared ? 1 : 0][cutout ? 1 : 0], dim3((tiles + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, view_or_dark(scene), cv);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_deferred_add_emissive(hr_deferred* deferred, const hr_image_view* emissive, void* stream)
{
    static const char* call = "hr_deferred_add_emissive";
    if (!deferred) return bad(call, "deferred is NULL");
    if (!emissive || !emissive->data) return bad(call, "emissive is NULL");
    hr_image_view colour;
    const hr_status s = hr_deferred_output(deferred, &colour);
    if (s != HR_OK) return s;
    if (emissive->format != HR_FORMAT_RGBA16F) return bad(call, "emissive is not RGBA16F");
    if (emissive->width != colour.width || emissive->height != colour.height || emissive->row_pitch_bytes != emissive->width * 8)
        return bad(call, "the emissive image does not match the pass's extent, tightly pitched");
    if (colour.format != HR_FORMAT_RGBA16F || colour.row_pitch_bytes != colour.width * 8) return bad(call, "the composite's output is not a tightly pitched RGBA16F image");
    HR_HIP(hipSetDevice(deferred_ctx(deferred)->device));
    const long long n = (long long)colour.width * colour.height;
    hipLaunchKernelGGL(k_add_emissive, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint2*)colour.data, (const uint2*)emissive->data, n);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

} // extern "C"
