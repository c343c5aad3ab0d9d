/* hr_probe_vis.h — the DDGI probe-grid visualisation (replaces DeferredShading::render_probes, deferred_shading.cpp:797-866, and
 * shaders/gi/gi_probe_visualization.vert/.frag, reached through set_visualize_probe_grid / set_probe_visualization_scale), C ABI.
 *
 * The reference rasterises one instanced sphere per probe over the composite, depth-tested against the G-buffer, and colours it from the
 * irradiance atlas at the sphere's normal.  Here every pixel's primary ray is intersected with the analytic spheres in one launch on the
 * caller's stream: no allocation, no host synchronisation, capturable into a hipGraph.  Nothing else in the library calls it.
 *
 * Library: hybrid_rendering_amd/libhybrid_rendering_amd.so (csrc/probe_vis.hip, device functions in csrc/probe_vis.h).  Every fp32
 * operation below is one correctly rounded operation, nothing is contracted, sums are taken in the order written.  dot3, sub3, normalize3,
 * mul_m4, world_pos_from_depth, hr_sqrt, __fdiv_rn, pack_h2 (csrc/device_math.h), grid_coord_to_position, texture_coord_from_direction,
 * atlas_bilinear_rgb and atlas_bilinear_rg (csrc/shading.h) are the library's own: what the DDGI gather computes with.
 */
#ifndef HR_PROBE_VIS_H
#define HR_PROBE_VIS_H

#include "hr_api.h"
#include "hr_api_post.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the contract ----------------------------------------------------------------------------------------------------------------------
 * Ray of pixel (x, y):  o = ubo.cam_pos.xyz;  d = normalize3(world_pos_from_depth((x + 0.5)/w, (y + 0.5)/h, 1, ubo.view_proj_inverse) - o):
 *   the ray hr_gbuffer_raycast traces through the pixel centre, so a sphere's depth is comparable with that G-buffer's.
 * Probe p = cx + cy*nx + cz*nx*ny (probe_index_to_grid_coord's inverse), centre c = grid_coord_to_position(grid, cx, cy, cz); r = radius.
 * Sphere test (d is unit length):
 *   oc = o - c;  b = dot3(oc, d);  q = oc - d*b (per component);  disc = r*r - dot3(q, q);  hit iff disc >= 0 (a NaN: no hit);
 *   t = -b - hr_sqrt(disc);  accepted iff t > 0.
 *   Front faces only — the reference culls back faces, a camera inside a sphere does not see it — and t > 0 stands for the near plane.
 * Winner: the smallest accepted t over ALL probes, on a tie the smallest p.
 * Depth test, on the winner only:  P = o + d*t;  clip = mul_m4(ubo.view_proj, P, 1);  z = clip.z / clip.w;
 *   drawn iff clip.w > 0 and z < depth_in[i]   (VK_COMPARE_OP_LESS with depth write).
 * Colour of a drawn texel:  n = normalize3(P - c);
 *   what == 0:  (u, v) = texture_coord_from_direction(n, p, irradiance_texture_width, irradiance_texture_height, irradiance_probe_side_length);
 *               rgb = atlas_bilinear_rgb(irradiance, u, v);  stored pack_h2, alpha 1                               (the reference)
 *   what == 1:  the same over the depth atlas's extents and side length;  g = atlas_bilinear_rg(...).mean / max_distance;  stored (g, g, g, 1).
 * A drawn texel:       color = the above,  depth_out = z,            probe_id_out = p.
 * Any other texel:     color keeps its bits, depth_out = depth_in[i], probe_id_out = -1.
 * The reference's sphere mesh is pinned to the unit sphere: radius = its probe_visualization_scale (0.5 at probe_distance 4, 5 at 50).
 * radius <= half the smallest grid_step walks the lattice; a larger one (overlapping spheres) tests every probe: the same answers, slower.
 */
typedef struct { float radius; int32_t what; } hr_probe_vis_params;   /* 8 bytes; default 0.5, 0 */
void      hr_probe_vis_default_params(hr_probe_vis_params* p);

/* Stateless, like hr_tone_map.  irradiance: the RGBA16F atlas; depth_atlas: the RG16F atlas, NULL unless what == 1; both with the extents `grid`
 * states, tightly pitched.  depth_in: device [h][w] fp32 ndc depth.  color: RGBA16F, drawn into in place; its extent is the image's.
 * depth_out: device [h][w], nullable, may alias depth_in.  probe_id_out: device [h][w] int32, nullable.
 * HR_ERR_INVALID_ARG before anything is enqueued: a NULL required pointer, a radius that is not finite or <= 0, what outside 0..1, what == 1
 * without a depth atlas, atlas extents or formats that disagree with grid, a probe_counts entry < 1, a color view that is not RGBA16F. */
hr_status hr_probe_vis_render(hr_ctx* ctx, const hr_ubo* ubo, const hr_ddgi_uniforms* grid, const hr_image_view* irradiance,
                              const hr_image_view* depth_atlas, const hr_probe_vis_params* params, const float* depth_in, hr_image_view* color,
                              float* depth_out, int32_t* probe_id_out, void* stream);

/* DeferredShading::render_probes: draws onto the pass's own output with ddgi's hr_ddgi_current_read atlases and hr_ddgi_get_uniforms, depth
 * from in->cur_full (as hr_deferred_render picks it; a level that does not match the pass's extent: HR_ERR_INVALID_ARG).  Call it after
 * hr_deferred_render on the same stream.  depth_out, handed on to what follows (TAA), is what the reference's depth write amounts to. */
hr_status hr_deferred_render_probes(hr_deferred* p, const hr_frame_inputs* in, hr_ddgi* ddgi, const hr_probe_vis_params* params,
                                    float* depth_out, int32_t* probe_id_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
