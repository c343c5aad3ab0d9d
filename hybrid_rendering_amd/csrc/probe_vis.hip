// DDGI probe-grid visualisation on MI355X — HIP replacement for DeferredShading::render_probes (deferred_shading.cpp:797-866,
// shaders/gi/gi_probe_visualization.vert/.frag): the reference rasterises one instanced sphere per probe over the composite with a depth
// test; here every pixel's primary ray is intersected with the analytic spheres.  Contract: include/hr_probe_vis.h.
#include "hr_internal.h"
#include "pixel_dir.h"
#include "probe_vis.h"
#include "../../include/hr_probe_vis.h"
#include <cmath>

using namespace hr;

struct ProbeVisArgs
{
    float        vpi[16], vp[16];
    float        cam[3];
    int          w, h;
    DDGIU        grid;
    float        inv_step[3]; // 1 / grid_step (fast only): candidate selection, never an output bit
    float        radius;
    int          what;
    int          fast;        // radius <= half the smallest step over a finite lattice: the plane walk; otherwise every probe
    AtlasRGBA    irradiance;
    AtlasRG      depth_atlas; // what == 1 only
    const float* depth_in;
    uint2*       color;
    float*       depth_out;   // nullable; may be depth_in
    int32_t*     probe_id_out;// nullable
};

// one wave = one 8x8 tile, as k_gbuffer_raycast
__global__ __launch_bounds__(256) void k_probe_vis(ProbeVisArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles_x = (a.w + 7) / 8, tiles_y = (a.h + 7) / 8;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= tiles_x * tiles_y) return;
    const int x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3);
    if (x >= a.w || y >= a.h) return;
    const size_t i  = (size_t)y * a.w + x;
    const f3     o  = mk3(a.cam[0], a.cam[1], a.cam[2]);
    const f3     d  = gb_pixel_dir(a, (float)x + 0.5f, (float)y + 0.5f);
    const float  di = a.depth_in[i];
    ProbeHit hit = probe_no_hit();
    if (a.fast)
    {
        const float slack = probe_walk_slack(a.grid, o, a.radius);
        // a tile none of whose rays reaches the grown box draws nothing: one vote, the same answer in every lane of the wave
        float t_exit;
        const bool in_box = probe_ray_hits_box(a.grid, o, d, slack, t_exit);
        if (__ballot(in_box) != 0ull && in_box) hit = probe_walk_planes(a.grid, a.inv_step, o, d, a.radius, slack, t_exit);
    }
    else hit = probe_walk_all(a.grid, o, d, a.radius);
    bool  drawn = false;
    float z = di;
    if (hit.p >= 0)
    {
        const f3 P = add3(o, scale3(d, hit.t));
        float zs;
        if (probe_depth_test(P, a.vp, di, zs))
        {
            const int cx = hit.p % a.grid.probe_counts[0];
            const int cy = (hit.p % (a.grid.probe_counts[0] * a.grid.probe_counts[1])) / a.grid.probe_counts[0];
            const int cz = hit.p / (a.grid.probe_counts[0] * a.grid.probe_counts[1]);
            const f3  n  = normalize3(sub3(P, grid_coord_to_position(a.grid, cx, cy, cz)));
            a.color[i] = probe_colour(a.grid, n, hit.p, a.what, a.irradiance, a.depth_atlas);
            drawn = true;
            z = zs;
        }
    }
    if (a.depth_out) a.depth_out[i] = z;
    if (a.probe_id_out) a.probe_id_out[i] = drawn ? hit.p : -1;
}

namespace {

hr_status refuse(const char* call, const char* what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

#define PV_REFUSE_IF(cond, what) do { if (cond) return refuse(call, what); } while (0)

// everything hr_probe_vis_render checks but the context; fills the launch arguments
hr_status probe_vis_args(const char* call, const hr_ubo* ubo, const hr_ddgi_uniforms* grid, const hr_image_view* irradiance, const hr_image_view* depth_atlas,
                         const hr_probe_vis_params* prm, const float* depth_in, hr_image_view* color, float* depth_out, int32_t* probe_id_out, ProbeVisArgs& a)
{
    PV_REFUSE_IF(!ubo, "ubo is NULL");
    PV_REFUSE_IF(!grid, "grid is NULL");
    PV_REFUSE_IF(!irradiance || !irradiance->data, "irradiance is NULL");
    PV_REFUSE_IF(!prm, "params is NULL");
    PV_REFUSE_IF(!depth_in, "depth_in is NULL");
    PV_REFUSE_IF(!color || !color->data, "color is NULL");
    PV_REFUSE_IF(!(std::isfinite(prm->radius) && prm->radius > 0.0f), "radius is not a finite positive number");
    PV_REFUSE_IF(prm->what < 0 || prm->what > 1, "what outside 0..1");
    PV_REFUSE_IF(prm->what == 1 && (!depth_atlas || !depth_atlas->data), "what == 1 needs the depth atlas");
    const DDGIU& g = *grid;
    PV_REFUSE_IF(g.probe_counts[0] < 1 || g.probe_counts[1] < 1 || g.probe_counts[2] < 1, "probe_counts below 1");
    PV_REFUSE_IF(g.probe_counts[0] > 1024 || g.probe_counts[1] > 1024 || g.probe_counts[2] > 1024 || (long long)g.probe_counts[0] * g.probe_counts[1] * g.probe_counts[2] > (1ll << 24),
                 "probe_counts above 1024 per axis or 2^24 probes");
    // the atlases are the grid's: the sizing of hr_ddgi_create, and a view that is what the grid says
    const int cols = g.probe_counts[0] * g.probe_counts[1], rows = g.probe_counts[2];
    PV_REFUSE_IF(g.irradiance_probe_side_length < 2 || g.irradiance_probe_side_length > 16 || g.irradiance_texture_width != (g.irradiance_probe_side_length + 2) * cols + 2 ||
                 g.irradiance_texture_height != (g.irradiance_probe_side_length + 2) * rows + 2, "irradiance atlas extents disagree with probe_counts");
    PV_REFUSE_IF(irradiance->format != HR_FORMAT_RGBA16F || irradiance->width != g.irradiance_texture_width || irradiance->height != g.irradiance_texture_height ||
                 irradiance->row_pitch_bytes != irradiance->width * 8, "irradiance view disagrees with the grid");
    if (prm->what == 1)
    {
        PV_REFUSE_IF(g.depth_probe_side_length < 2 || g.depth_probe_side_length > 16 || g.depth_texture_width != (g.depth_probe_side_length + 2) * cols + 2 ||
                     g.depth_texture_height != (g.depth_probe_side_length + 2) * rows + 2, "depth atlas extents disagree with probe_counts");
        PV_REFUSE_IF(depth_atlas->format != HR_FORMAT_RG16F || depth_atlas->width != g.depth_texture_width || depth_atlas->height != g.depth_texture_height ||
                     depth_atlas->row_pitch_bytes != depth_atlas->width * 4, "depth atlas view disagrees with the grid");
    }
    PV_REFUSE_IF(color->format != HR_FORMAT_RGBA16F, "color is not RGBA16F");
    PV_REFUSE_IF(color->width < 1 || color->height < 1 || color->row_pitch_bytes != color->width * 8, "color extent");
    for (int k = 0; k < 16; k++) { a.vpi[k] = ubo->view_proj_inverse[k]; a.vp[k] = ubo->view_proj[k]; }
    for (int k = 0; k < 3; k++) a.cam[k] = ubo->cam_pos[k];
    a.w = color->width; a.h = color->height;
    a.grid = g; a.radius = prm->radius; a.what = prm->what;
    bool lattice_ok = true;
    float min_step = INFINITY;
    for (int k = 0; k < 3; k++)
    {
        lattice_ok = lattice_ok && std::isfinite(g.grid_start_position[k]) && std::isfinite(g.grid_step[k]) && g.grid_step[k] > 0.0f && std::isfinite(1.0f / g.grid_step[k]);
        min_step = g.grid_step[k] < min_step ? g.grid_step[k] : min_step;
    }
    a.fast = lattice_ok && prm->radius <= 0.5f * min_step ? 1 : 0;
    for (int k = 0; k < 3; k++) a.inv_step[k] = a.fast ? 1.0f / g.grid_step[k] : 0.0f;
    a.irradiance = AtlasRGBA { (const uint2*)irradiance->data, irradiance->width, irradiance->height };
    a.depth_atlas = prm->what == 1 ? AtlasRG { (const uint32_t*)depth_atlas->data, depth_atlas->width, depth_atlas->height } : AtlasRG { nullptr, 0, 0 };
    a.depth_in = depth_in; a.color = (uint2*)color->data; a.depth_out = depth_out; a.probe_id_out = probe_id_out;
    return HR_OK;
}

hr_status probe_vis_launch(hr_ctx* ctx, const ProbeVisArgs& a, void* stream)
{
    HR_SCOPED_SAMPLE("DDGI Visualize Probe Grid");
    HR_HIP(hipSetDevice(ctx->device));
    const int tiles = ((a.w + 7) / 8) * ((a.h + 7) / 8);
    hipLaunchKernelGGL(k_probe_vis, dim3((tiles + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

} // namespace

extern "C" {

void hr_probe_vis_default_params(hr_probe_vis_params* p)
{
    if (!p) return;
    p->radius = 0.5f;
    p->what   = 0;
}

hr_status hr_probe_vis_render(hr_ctx* ctx, const hr_ubo* ubo, const hr_ddgi_uniforms* grid, const hr_image_view* irradiance, const hr_image_view* depth_atlas,
                              const hr_probe_vis_params* prm, const float* depth_in, hr_image_view* color, float* depth_out, int32_t* probe_id_out, void* stream)
{
    const char* call = "hr_probe_vis_render";
    ProbeVisArgs a;
    const hr_status s = probe_vis_args(call, ubo, grid, irradiance, depth_atlas, prm, depth_in, color, depth_out, probe_id_out, a);
    if (s != HR_OK) return s;
    PV_REFUSE_IF(!ctx, "ctx is NULL");   // last: what was handed in is judged without a device
    return probe_vis_launch(ctx, a, stream);
}

hr_status hr_deferred_render_probes(hr_deferred* p, const hr_frame_inputs* in, hr_ddgi* ddgi, const hr_probe_vis_params* prm, float* depth_out, int32_t* probe_id_out, void* stream)
{
    const char* call = "hr_deferred_render_probes";
    PV_REFUSE_IF(!p, "deferred is NULL");
    PV_REFUSE_IF(!in, "in is NULL");
    PV_REFUSE_IF(!ddgi, "ddgi is NULL");
    hr_image_view    color, irradiance, depth_atlas;
    hr_ddgi_uniforms grid;
    hr_status s;
    if ((s = hr_deferred_output(p, &color)) != HR_OK || (s = hr_ddgi_current_read(ddgi, &irradiance, &depth_atlas)) != HR_OK || (s = hr_ddgi_get_uniforms(ddgi, &grid)) != HR_OK) return s;
    const hr_gbuffer_level& g = in->cur_full.gb2 ? in->cur_full : in->cur;   // as hr_deferred_render picks it
    PV_REFUSE_IF(!g.depth || g.width != color.width || g.height != color.height, "the G-buffer level does not match the pass's extent");
    ProbeVisArgs a;
    if ((s = probe_vis_args(call, &in->ubo, &grid, &irradiance, &depth_atlas, prm, g.depth, &color, depth_out, probe_id_out, a)) != HR_OK) return s;
    return probe_vis_launch(deferred_ctx(p), a, stream);
}

} // extern "C"
