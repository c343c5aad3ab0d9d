// Extra lights: the scene's light list (host side) and the primary-surface pass hr_lights (contract: include/hr_lights.h).  The list's term in the
// hit shaders is lights.h, called by the LIGHTS instantiations of ddgi.hip, reflections.hip and ground_truth.hip.
//
// The setters follow hr_scene_set_emission (emission.hip): host state read when a pass enqueues, one device table allocated by the first setter
// call, the host form staged through pinned memory the scene owns (the next call waits for the copy's event before it rewrites the staging).
// The arguments are checked against host state alone, before the device is touched.
#include "lights_host.h"
#include "cutout_host.h"
#include "instances_shared_device.h"
#include "../../include/hr_lights.h"
#include <cmath>
#include <cstring>

using namespace hr;

namespace {

// ---- hr_lights_render ----------------------------------------------------------------------------------------------------------------------
struct LightsPassArgs
{
    float           vpi[16];
    float           cam[3];
    const uint32_t* gb1;
    const uint2*    gb2;
    const uint2*    gb3;
    const float*    depth;
    const Node8*    nodes;
    const TriGPU*   tris;
    SceneShading    sh;
    uint2*          out;
    int             w, h, tiles_x, tiles_y;
    float           bias;
};

// One wave = one 8x8 tile, one workgroup per wave, as in the shadow trace (tile costs differ widely: single-wave groups let the dispatcher
// back-fill a CU wave by wave).  The G-buffer texel is decoded ONCE, with k_deferred's operations (deferred.hip), outside the loop over the
// lights; a light's record is one wave-uniform load (lights.h LightsView); the per-lane any-hit walk (trace_any / trace_any2 through
// visibility_ray_occluded, the LDS stack they always use) runs only in waves where some lane has attenuation > 0 for that light.
// No lane leaves early: a lane outside the image or on a sky texel carries `surf == false`, fires no ray and adds nothing.
// A skipped walk is exact: vis is only ever read as 1 where no ray is traced, which is the contract's own rule.
template <bool SHARED, bool CUTOUT>
__global__ __launch_bounds__(64) void k_lights_primary(LightsPassArgs a, LightsView lt, CutoutView cv)
{
    __shared__ uint32_t s_stack[HR_STACK_ENTRIES * 64];
    const int lane = threadIdx.x;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool   inside = x < a.w && y < a.h;
    const size_t i      = inside ? (size_t)y * a.w + x : 0;   // a lane outside the image reads texel 0 and ignores it
    const float    dp = a.depth[i];
    const uint32_t g1 = a.gb1[i];
    const uint2    g2 = a.gb2[i], g3 = a.gb3[i];
    const bool     surf = inside && dp != 1.0f;
    // k_deferred's decode (deferred.hip:41-53)
    const float tu = __fdiv_rn((float)x + 0.5f, (float)a.w), tv = __fdiv_rn((float)y + 0.5f, (float)a.h);
    const f3    albedo   = mk3(__fdiv_rn((float)(g1 & 0xffu), 255.0f), __fdiv_rn((float)((g1 >> 8) & 0xffu), 255.0f), __fdiv_rn((float)((g1 >> 16) & 0xffu), 255.0f));
    const float metallic = __fdiv_rn((float)(g1 >> 24), 255.0f);
    const float roughness = h2f_lo(g3.x);
    const f3    P  = world_pos_from_depth(tu, tv, dp, a.vpi);
    const f3    N  = oct_decode(h2f_lo(g2.x), h2f_hi(g2.x));
    const f3    Wo = normalize3(sub3(mk3(a.cam[0], a.cam[1], a.cam[2]), P));
    const f3    F0 = mix3(mk3(0.04f, 0.04f, 0.04f), albedo, metallic);
    const f3    c_diffuse = mix3(mul3(albedo, sub3(one3(), F0)), mk3(0.0f, 0.0f, 0.0f), metallic);
    const f3    ray_origin = add3(P, scale3(N, a.bias));
    TraceCtxOf<SHARED> tc = make_trace_ctx<SHARED>(a.nodes, a.tris, a.sh, s_stack, lane);
    if constexpr (CUTOUT) tc.cv = cv;
    f3       sum = mk3(0.0f, 0.0f, 0.0f);
    uint32_t nn = 0, nt = 0;
    for (int k = 0; k < lt.n; k++)
    {
        const hr_light L = lt.table[k];
        f3    Li, Wi, Wh;
        float t_max, attenuation;
        fetch_light_hard(L, Wo, P, N, Li, Wi, Wh, t_max, attenuation);
        const bool fire = surf && attenuation > 0.0f;
        float      vis  = 1.0f;
        if (__ballot(fire) != 0ull)   // wave-uniform: no lane of the tile faces this light, or is in its cone: no walk
        {
            if (fire) vis = visibility_ray_occluded<false, CUTOUT>(tc, ray_origin, Wi, 0.01f, t_max, nn, nt) ? 0.0f : 1.0f;
        }
        const f3 brdf = evaluate_uber_brdf(c_diffuse, roughness, N, F0, Wo, Wh, Wi);
        // the composite's expression (deferred.hip:60), vis where the shadow image was
        const f3 term = scale3(mul3(scale3(mul3(one3(), brdf), attenuation), Li), vis);
        if (surf) sum = add3(sum, term);
    }
    if (inside) a.out[i] = surf ? make_uint2(pack_h2(sum.x, sum.y), pack_h2(sum.z, 1.0f)) : make_uint2(0u, 0u);
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

// the first setter call: the table of HR_MAX_LIGHTS records (zeroed: a record the host never set is a directional light of intensity 0), the
// pinned staging and its event.  All or none: lights_stage, set last, is what says "allocated".  Synchronous, like creation.
hr_status ensure_table(hr_scene* s, const char* call, hipStream_t st)
{
    if (s->lights_stage) return HR_OK;
    HR_HIP(hipSetDevice(s->ctx->device));
    if (stream_is_capturing(st)) return bad(call, "the first call allocates: not possible while the stream is capturing");
    const size_t bytes = (size_t)HR_MAX_LIGHTS * sizeof(hr_light);
    hr_light*  stage = nullptr;
    hipEvent_t done = nullptr;
    hr_status  e = s->lights_dev.alloc(bytes);
    if (e == HR_OK && hipMemset(s->lights_dev.p, 0, bytes) != hipSuccess) { set_last_error(std::string(call) + ": hipMemset failed"); e = HR_ERR_HIP; }
    if (e == HR_OK && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) { done = nullptr; set_last_error(std::string(call) + ": hipEventCreateWithFlags failed"); e = HR_ERR_HIP; }
    if (e == HR_OK && hipHostMalloc((void**)&stage, bytes, hipHostMallocDefault) != hipSuccess) { stage = nullptr; set_last_error(std::string(call) + ": hipHostMalloc failed"); e = HR_ERR_OUT_OF_MEMORY; }
    if (e != HR_OK)
    {
        (void)hipGetLastError();
        if (done) (void)hipEventDestroy(done);
        s->lights_dev.free();
        return e;
    }
    s->lights_copied = done;
    s->lights_stage = stage;
    return HR_OK;
}

// null: the light is acceptable; else what is wrong with it
const char* light_fault(const hr_light& L)
{
    const float* f = L.data0;   // the four rows are contiguous: 16 floats
    static_assert(sizeof(hr_light) == 64, "hr_light is four rows of four floats");
    for (int c = 0; c < 16; c++)
        if (!std::isfinite(f[c])) return "has a component that is not finite";
    if (!(L.data3[0] == 0.0f || L.data3[0] == 1.0f || L.data3[0] == 2.0f)) return "has a type (data3[0]) that is not 0, 1 or 2";
    if (L.data0[3] < 0.0f) return "has a negative intensity (data0[3])";
    if (L.data1[3] < 0.0f) return "has a negative radius (data1[3])";
    return nullptr;
}

hr_status set_lights(hr_scene* s, const hr_light* lights, int32_t n, hipStream_t st)
{
    static const char* call = "hr_scene_set_lights";
    if (!s) return bad(call, "scene is NULL");
    if (n < 0 || n > HR_MAX_LIGHTS) return bad(call, "n = " + std::to_string(n) + " is outside 0 .. HR_MAX_LIGHTS (" + std::to_string(HR_MAX_LIGHTS) + ")");
    if (n > 0 && !lights) return bad(call, "host_lights is NULL");
    for (int k = 0; k < n; k++)
        if (const char* what = light_fault(lights[k])) return bad(call, "light " + std::to_string(k) + " " + what);
    if (n == 0) { s->lights_host.clear(); return HR_OK; }   // off: the table, if there is one, is no longer read
    std::vector<hr_light> copy(lights, lights + n);         // before anything changes: the one allocation that may throw
    const hr_status e = ensure_table(s, call, st);
    if (e != HR_OK) return e;
    if (stream_is_capturing(st)) return bad(call, "stages through memory the next call rewrites: not possible while the stream is capturing");
    HR_HIP(hipEventSynchronize(s->lights_copied));   // the staging may still feed the previous call's copy
    std::memcpy(s->lights_stage, lights, (size_t)n * sizeof(hr_light));
    HR_HIP(hipMemcpyAsync(s->lights_dev.p, s->lights_stage, (size_t)n * sizeof(hr_light), hipMemcpyHostToDevice, st));
    HR_HIP(hipEventRecord(s->lights_copied, st));
    s->lights_host.swap(copy);
    return HR_OK;
}

hr_status set_lights_device(hr_scene* s, const hr_light* dev, hipStream_t st)
{
    static const char* call = "hr_scene_set_lights_device";
    if (!s) return bad(call, "scene is NULL");
    const size_t n = s->lights_host.size();
    if (n > 0 && !dev) return bad(call, "dev_lights is NULL");
    const hr_status e = ensure_table(s, call, st);
    if (e != HR_OK) return e;
    if (n > 0) HR_HIP(hipMemcpyAsync(s->lights_dev.p, dev, n * sizeof(hr_light), hipMemcpyDeviceToDevice, st));
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

bool hr::reject_lights_dev_switches(const hr_scene* s, const char* call, bool wanted)
{
    if (!wanted || !lights_live(s)) return false;
    set_last_error(std::string(call) + ": trace statistics and developer switches are not available while the scene has a light list (hr_scene_set_lights)");
    return true;
}

struct hr_lights
{
    hr_ctx* ctx = nullptr;
    int     w = 0, h = 0;
    DevBuf  out;
};

extern "C" {

hr_status hr_scene_set_lights(hr_scene* scene, const hr_light* host_lights, int32_t n, void* stream)
{
    return no_throw("hr_scene_set_lights", [&] { return set_lights(scene, host_lights, n, (hipStream_t)stream); });
}

hr_status hr_scene_set_lights_device(hr_scene* scene, const hr_light* dev_lights, void* stream)
{
    return no_throw("hr_scene_set_lights_device", [&] { return set_lights_device(scene, dev_lights, (hipStream_t)stream); });
}

hr_status hr_scene_get_lights(const hr_scene* scene, hr_light* host_out, int32_t* n)
{
    static const char* call = "hr_scene_get_lights";
    if (!scene) return bad(call, "scene is NULL");
    if (!host_out && !n) return bad(call, "host_out and n are both NULL");
    if (n) *n = (int32_t)scene->lights_host.size();
    if (host_out && !scene->lights_host.empty()) std::memcpy(host_out, scene->lights_host.data(), scene->lights_host.size() * sizeof(hr_light));
    return HR_OK;
}

void hr_lights_default_params(hr_lights_params* p)
{
    hr_shadows_params sp;
    hr_shadows_default_params(&sp);
    p->bias = sp.bias;
}

hr_status hr_lights_create(hr_ctx* ctx, int32_t width, int32_t height, hr_lights** out)
{
    HR_CHECK_ARG(ctx && out && width > 0 && height > 0);
    HR_HIP(hipSetDevice(ctx->device));
    hr_lights* p = new hr_lights();
    p->ctx = ctx; p->w = width; p->h = height;
    const hr_status s = p->out.alloc((size_t)width * height * 8);
    if (s != HR_OK) { delete p; return s; }
    *out = p;
    return HR_OK;
}

hr_status hr_lights_destroy(hr_lights* p)
{
    if (!p) return HR_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipDeviceSynchronize();
    delete p;
    return HR_OK;
}

hr_status hr_lights_render(hr_lights* p, const hr_scene* scene, const hr_frame_inputs* in, const hr_lights_params* prm, void* stream)
{
    static const char* call = "hr_lights_render";
    HR_CHECK_ARG(p && scene && in);
    const hr_gbuffer_level& g = in->cur_full.gb2 ? in->cur_full : in->cur;
    HR_CHECK_ARG(g.gb1 && g.gb2 && g.gb3 && g.depth && g.width == p->w && g.height == p->h);
    hr_lights_params def;
    hr_lights_default_params(&def);
    const float bias = prm ? prm->bias : def.bias;
    if (!std::isfinite(bias)) return bad(call, "bias is not finite");
    HR_HIP(hipSetDevice(p->ctx->device));
    LightsPassArgs a;
    for (int i = 0; i < 16; i++) a.vpi[i] = in->ubo.view_proj_inverse[i];
    for (int i = 0; i < 3; i++) a.cam[i] = in->ubo.cam_pos[i];
    a.gb1 = (const uint32_t*)g.gb1; a.gb2 = (const uint2*)g.gb2; a.gb3 = (const uint2*)g.gb3; a.depth = g.depth;
    a.nodes = (const Node8*)scene->nodes.p; a.tris = (const TriGPU*)scene->tris.p;
    scene_shading_from(scene, a.sh);
    a.out = (uint2*)p->out.p;
    a.w = p->w; a.h = p->h; a.tiles_x = cdiv(p->w, 8); a.tiles_y = cdiv(p->h, 8);
    a.bias = bias;
    // an empty list: n = 0 and no table — the loop does not run and every surface texel is (0, 0, 0, 1)
    LightsView lt;
    lt.table = lights_live(scene) ? (const hr_light*)scene->lights_dev.p : nullptr;
    lt.n     = (int)scene->lights_host.size();
    const bool       cutout = cutout_on(scene, HR_RAY_SHADOW);
    const CutoutView cv = cutout ? cutout_view_of(scene) : CutoutView();
    void (*const kernel[2][2])(LightsPassArgs, LightsView, CutoutView) = { { k_lights_primary<false, false>, k_lights_primary<false, true> },
                                                                           { k_lights_primary<true, false>, k_lights_primary<true, true> } };
    hipLaunchKernelGGL(kernel[scene->shared ? 1 : 0][cutout ? 1 : 0], dim3((unsigned)(a.tiles_x * a.tiles_y)), dim3(64), 0, (hipStream_t)stream, a, lt, cv);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_lights_output(hr_lights* p, hr_image_view* v)
{
    HR_CHECK_ARG(p && v);
    v->data = p->out.p; v->width = p->w; v->height = p->h; v->row_pitch_bytes = p->w * 8; v->format = HR_FORMAT_RGBA16F;
    return HR_OK;
}

} // extern "C"
