// GroundTruthPathTracer on MI355X — HIP replacement for src/ground_truth_path_tracer.cpp (render :44-111) and
// shaders/ground_truth/ground_truth_path_trace.{rgen:52-112, rchit:114-142, rmiss:24-32}.  SURVEY.md §8f row 3.
// One wave = one 8x8 pixel tile, one lane = one pixel: jittered primary ray (closest hit), direct lighting at the hit
// (punctual light with soft shadows + one cosine-lobe sky sample, each with a visibility ray), running mean into the
// ping-pong RGBA16F images.  indirect_lighting (rchit:67-108) contributes nothing upstream — its recursive traceRayEXT
// is commented out (rchit:95-105) and p_IndirectPayload.L stays 0.  hr_ground_truth_params.trace_indirect = 1 re-enables
// that call (SURVEY §8f row 3's optional extension): up to max_ray_bounces path segments with Russian roulette.
#include "hr_internal.h"
#include "shading.h"
#include "cutout_host.h"
#include "emission_host.h"
#include "lights_host.h"

using namespace hr;

struct GTArgs
{
    float        view_inverse[16], proj_inverse[16];
    hr_light     light;
    const Node8* nodes;
    const TriGPU* tris;
    SceneShading sh;
    CubeMap      sky;
    const uint2* prev;
    uint2*       cur;
    uint32_t*    ray_slots;   // rays per 8x8 tile
    int          w, h, y0, y1, tiles_x, tile_y0;
    uint32_t     num_frames;
    float        roughness_multiplier;
    uint32_t     max_ray_bounces;
    int          trace_indirect;
};

#define GT_MAX_DEPTH 32
// sample_specular_ggx_lobe (brdf.glsl:96-112): sampling.h

// INDIRECT = false is the reference as shipped (one invocation per pixel: no payload chain to keep)
// SHARED: every bounce and every visibility ray over a shared instanced scene (a.sh.inst_shared set) — the two-level walk of traverse2.h
// CUTOUT: the camera ray (class HR_RAY_PRIMARY, cv_primary), the bounces (HR_RAY_GI, cv_gi) and the visibility rays (HR_RAY_SHADOW, cv_shadow) run the
// alpha test of cutout.h; the host picks it iff any of the three classes has cutouts on, and hands the others a view without a table.
// EMISSIVE (emission.h; hr_scene_set_emission): Lo = Lo + T * E at every hit of the chain, before adds[depth] = Lo and so before RADIANCE_CLAMP_COLOR; at
// depth 0 the throughput is 1 and the product is skipped, as for the sky.  The kernels that existed before it keep their names, their arguments
// and their code: the body is ground_truth_body.h, included into both.
#define HR_GROUND_TRUTH_BODY   // ground_truth_body.h refuses any other includer
template <bool INDIRECT, bool SHARED = false, bool CUTOUT = false>
__global__ __launch_bounds__(64) void k_ground_truth(GTArgs a, CutoutView cv_primary, CutoutView cv_gi, CutoutView cv_shadow)
{
    constexpr bool     EMISSIVE = false, LIGHTS = false;
    [[maybe_unused]] const EmissionView em = EmissionView();   // never read
    [[maybe_unused]] const LightsView   lt = LightsView();     // never read
#include "ground_truth_body.h"
}
template <bool INDIRECT, bool SHARED, bool CUTOUT>
__global__ __launch_bounds__(64) void k_ground_truth_emissive(GTArgs a, CutoutView cv_primary, CutoutView cv_gi, CutoutView cv_shadow, EmissionView em)
{
    constexpr bool EMISSIVE = true, LIGHTS = false;
    [[maybe_unused]] const LightsView lt = LightsView();   // never read
#include "ground_truth_body.h"
}
// LIGHTS (lights.h; hr_scene_set_lights): Lo = Lo + X at every hit of the chain, after the sky block and before emission; the list's terms take the
// hit's T and the two numbers the UBO light drew.  One kernel with and without live emission (lights_host.h emission_view_or_none).
template <bool INDIRECT, bool SHARED, bool CUTOUT>
__global__ __launch_bounds__(64) void k_ground_truth_lights(GTArgs a, CutoutView cv_primary, CutoutView cv_gi, CutoutView cv_shadow, EmissionView em, LightsView lt)
{
    constexpr bool EMISSIVE = true, LIGHTS = true;
#include "ground_truth_body.h"
}
#undef HR_GROUND_TRUTH_BODY

struct hr_ground_truth
{
    hr_ctx*  ctx = nullptr;
    int      w = 0, h = 0, y0 = 0, y1 = 0, tiles_x = 0;
    DevBuf   image[2], ray_slots;
    uint32_t frame_idx = 0;
    bool     ping_pong = false;
    hipStream_t last_stream = nullptr;
    StageProfiler prof;
};

extern "C" {

void hr_ground_truth_default_params(hr_ground_truth_params* p)
{
    p->max_ray_bounces = 2;         // ground_truth_path_tracer.h:30
    p->roughness_multiplier = 1.0f; // CommonResources::roughness_multiplier
    p->trace_indirect = 0;          // the reference ships the recursive trace commented out (rchit:95-105)
}

hr_status hr_ground_truth_create(hr_ctx* ctx, int32_t width, int32_t height, const hr_band* band, hr_ground_truth** out)
{
    HR_CHECK_ARG(ctx && out && width > 0 && height > 0);
    HR_HIP(hipSetDevice(ctx->device));
    hr_ground_truth* p = new hr_ground_truth();
    p->ctx = ctx; p->w = width; p->h = height; p->y0 = 0; p->y1 = height;
    if (band && band->band_y1 > band->band_y0)
    {
        // pixels are independent: a band needs no halo and no exchange
        p->y0 = band->band_y0; p->y1 = band->band_y1 > height ? height : band->band_y1;
        if ((p->y0 & 7) || p->y0 < 0 || p->y0 >= p->y1) { set_last_error("band_y0 must be a multiple of 8 inside the image"); delete p; return HR_ERR_INVALID_ARG; }
    }
    p->tiles_x = cdiv(width, 8);
    hr_status s;
    for (int i = 0; i < 2; i++)
    {
        if ((s = p->image[i].alloc((size_t)width * height * 8)) != HR_OK) { delete p; return s; }
        HR_HIP(hipMemset(p->image[i].p, 0, p->image[i].bytes));
    }
    if ((s = p->ray_slots.alloc((size_t)p->tiles_x * cdiv(height, 8) * 4)) != HR_OK) { delete p; return s; }
    HR_HIP(hipMemset(p->ray_slots.p, 0, p->ray_slots.bytes));
    *out = p;
    return HR_OK;
}

hr_status hr_ground_truth_destroy(hr_ground_truth* p)
{
    if (!p) return HR_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipDeviceSynchronize();
    delete p;
    return HR_OK;
}

hr_status hr_ground_truth_restart_accumulation(hr_ground_truth* p) { HR_CHECK_ARG(p); p->frame_idx = 0; return HR_OK; }
hr_status hr_ground_truth_set_profiling(hr_ground_truth* p, int32_t e) { HR_CHECK_ARG(p); p->prof.enabled = e != 0; return HR_OK; }
hr_status hr_ground_truth_get_stage_times(hr_ground_truth* p, hr_stage_times* out) { HR_CHECK_ARG(p && out); p->prof.collect(out); return HR_OK; }

hr_status hr_ground_truth_render(hr_ground_truth* p, const hr_scene* scene, const hr_ubo* ubo, const hr_environment* env, const hr_ground_truth_params* prm, void* stream_)
{
    HR_CHECK_ARG(p && scene && ubo && env && prm && env->sky && env->sky_size > 0);
    HR_REJECT_SHARED(scene, "hr_ground_truth_render");
    HR_HIP(hipSetDevice(p->ctx->device));
    hipStream_t st = (hipStream_t)stream_;
    p->last_stream = st;
    p->prof.begin_frame();
    if (p->frame_idx == 0) p->ping_pong = false; // ground_truth_path_tracer.cpp:50-51
    const int read_idx = p->ping_pong ? 1 : 0, write_idx = p->ping_pong ? 0 : 1;
    GTArgs a;
    for (int i = 0; i < 16; i++) { a.view_inverse[i] = ubo->view_inverse[i]; a.proj_inverse[i] = ubo->proj_inverse[i]; }
    a.light = ubo->light;
    a.nodes = (const Node8*)scene->nodes.p; a.tris = (const TriGPU*)scene->tris.p;
    scene_shading_from(scene, a.sh);
    a.sky = CubeMap { (const uint2*)env->sky, env->sky_size };
    a.prev = (const uint2*)p->image[read_idx].p; a.cur = (uint2*)p->image[write_idx].p;
    a.ray_slots = (uint32_t*)p->ray_slots.p;
    a.w = p->w; a.h = p->h; a.y0 = p->y0; a.y1 = p->y1; a.tiles_x = p->tiles_x; a.tile_y0 = p->y0 / 8;
    a.num_frames = p->frame_idx++;
    a.roughness_multiplier = prm->roughness_multiplier;
    a.max_ray_bounces = (uint32_t)prm->max_ray_bounces; a.trace_indirect = prm->trace_indirect ? 1 : 0;
    const int tiles_y = cdiv(p->y1, 8) - a.tile_y0;
    const uint64_t px = (uint64_t)p->w * (p->y1 - p->y0);
    int ev = p->prof.begin("path_trace", st, px * 16);
    // one CUTOUT instantiation for the three classes the kernel fires; a class that is forced opaque gets a view without a table
    const bool cut_primary = cutout_on(scene, HR_RAY_PRIMARY), cut_gi = cutout_on(scene, HR_RAY_GI), cut_shadow = cutout_on(scene, HR_RAY_SHADOW);
    const CutoutView off = CutoutView(), on = (cut_primary || cut_gi || cut_shadow) ? cutout_view_of(scene) : off;
    void (*const kernel[2][2][2])(GTArgs, CutoutView, CutoutView, CutoutView) = { { { k_ground_truth<false, false, false>, k_ground_truth<false, false, true> }, { k_ground_truth<false, true, false>, k_ground_truth<false, true, true> } },
                                                                                  { { k_ground_truth<true, false, false>, k_ground_truth<true, false, true> }, { k_ground_truth<true, true, false>, k_ground_truth<true, true, true> } } };
    // ... and the EMISSIVE ones, picked iff the scene's emission is enabled and some material emits (hr_internal.h emission_live)
    void (*const emissive[2][2][2])(GTArgs, CutoutView, CutoutView, CutoutView, EmissionView) = {
        { { k_ground_truth_emissive<false, false, false>, k_ground_truth_emissive<false, false, true> }, { k_ground_truth_emissive<false, true, false>, k_ground_truth_emissive<false, true, true> } },
        { { k_ground_truth_emissive<true, false, false>, k_ground_truth_emissive<true, false, true> }, { k_ground_truth_emissive<true, true, false>, k_ground_truth_emissive<true, true, true> } } };
    // ... and the LIGHTS ones, picked iff the scene's light list is not empty (hr_internal.h lights_live)
    void (*const lights[2][2][2])(GTArgs, CutoutView, CutoutView, CutoutView, EmissionView, LightsView) = {
        { { k_ground_truth_lights<false, false, false>, k_ground_truth_lights<false, false, true> }, { k_ground_truth_lights<false, true, false>, k_ground_truth_lights<false, true, true> } },
        { { k_ground_truth_lights<true, false, false>, k_ground_truth_lights<true, false, true> }, { k_ground_truth_lights<true, true, false>, k_ground_truth_lights<true, true, true> } } };
    if (lights_live(scene))
        hipLaunchKernelGGL(lights[a.trace_indirect ? 1 : 0][scene->shared ? 1 : 0][cut_primary || cut_gi || cut_shadow], dim3(p->tiles_x * tiles_y), dim3(64), 0, st, a,
                           cut_primary ? on : off, cut_gi ? on : off, cut_shadow ? on : off, emission_view_or_none(scene), lights_view_of(scene));
    else if (emission_live(scene))
        hipLaunchKernelGGL(emissive[a.trace_indirect ? 1 : 0][scene->shared ? 1 : 0][cut_primary || cut_gi || cut_shadow], dim3(p->tiles_x * tiles_y), dim3(64), 0, st, a,
                           cut_primary ? on : off, cut_gi ? on : off, cut_shadow ? on : off, emission_view_of(scene));
    else
        hipLaunchKernelGGL(kernel[a.trace_indirect ? 1 : 0][scene->shared ? 1 : 0][cut_primary || cut_gi || cut_shadow], dim3(p->tiles_x * tiles_y), dim3(64), 0, st, a,
                           cut_primary ? on : off, cut_gi ? on : off, cut_shadow ? on : off);
    p->prof.end(ev, st);
    HR_HIP(hipGetLastError());
    p->ping_pong = !p->ping_pong;
    return HR_OK;
}

// GroundTruthPathTracer::output_ds: the image written by the last render()
hr_status hr_ground_truth_output(hr_ground_truth* p, hr_image_view* v)
{
    HR_CHECK_ARG(p && v);
    const int last_write = p->ping_pong ? 1 : 0; // render() flipped ping_pong after writing !ping_pong
    v->data = p->image[last_write].p; v->width = p->w; v->height = p->h; v->row_pitch_bytes = p->w * 8; v->format = HR_FORMAT_RGBA16F;
    return HR_OK;
}

hr_status hr_ground_truth_ray_count(hr_ground_truth* p, uint64_t* rays)
{
    HR_CHECK_ARG(p && rays);
    HR_HIP(hipStreamSynchronize(p->last_stream));
    std::vector<uint32_t> slots(p->ray_slots.bytes / 4);
    HR_HIP(hipMemcpy(slots.data(), p->ray_slots.p, slots.size() * 4, hipMemcpyDeviceToHost));
    uint64_t total = 0;
    const int t0 = (p->y0 / 8) * p->tiles_x, t1 = cdiv(p->y1, 8) * p->tiles_x;
    for (int i = 0; i < t1 - t0; i++) total += slots[i];
    *rays = total;
    return HR_OK;
}

} // extern "C"
