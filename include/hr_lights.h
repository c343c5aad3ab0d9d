/* hr_lights.h — extra lights: a per-scene light list in every hit shader and on the primary surfaces, C ABI.
 *
 * Every pass takes one light, hr_ubo.light, because the reference's UBO carries one Light (src/common.h:161-179).  This header is where the
 * library goes past it: a scene may carry a LIST of up to HR_MAX_LIGHTS further hr_light records.  The list is OPT-IN per scene and EMPTY by
 * default: with it empty every launch takes the kernel and the arguments it took before this header existed, bit for bit.  No struct of
 * hr_api.h changes.
 *
 * Library: hybrid_rendering_amd/libhybrid_rendering_amd.so (csrc/lights.hip; the per-light term of the hit shaders is csrc/lights.h, one text
 * for the three trace kernels).  Every fp32 operation below is one correctly rounded operation, nothing is contracted, sums are taken in the
 * order written.
 *
 * Out of scope: soft or denoised shadows for list lights on primary surfaces (a caller who wants them runs a second hr_shadows under that
 * light); a stage inside hr_hybrid_frame (the frame's passes read the list through the scene, the primary pass is run by the caller);
 * row-band tiling of hr_lights; light culling or a range.
 */
#ifndef HR_LIGHTS_H
#define HR_LIGHTS_H

#include "hr_api.h"
#include "hr_api_post.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_MAX_LIGHTS 256

/* ---- the contract ----------------------------------------------------------------------------------------------------------------------
 * At a hit with position P, shading normal N, outgoing direction Wo, throughput T and the hit shader's F0, diffuse colour and roughness:
 *   t_k = exactly what direct_lighting's first block (lighting.glsl:117-160) computes for its light, with light k of the list in the UBO
 *         light's place: fetch_light_properties without SOFT_SHADOWS; where attenuation > 0 one any-hit ray from P + N * 0.1 over
 *         [0.01, t_max), of class HR_RAY_SHADOW, through the same cutout view, attenuation = attenuation * (occluded ? 0 : 1);
 *         t_k = ((T * brdf) * attenuation) * Li.
 *   X   = ((+0 + t_0) + t_1) + ..., in list order.
 *   hr_ddgi_ray_trace          Lo = direct_lighting(...) + X     before the infinite-bounce term and before emission's E
 *   hr_reflections_ray_trace   hLo = direct_lighting(...) + X    at a hit; rough pixels that take the DDGI approximation get nothing, as ever
 *   hr_ground_truth_render     t_k uses the SOFT_SHADOWS fetch (radius, the disc sample) with the two numbers r1x, r1y the UBO light already
 *                              drew at that hit — the list draws nothing from the RNG, so the path is unchanged — and the same T;
 *                              Lo = Lo + X after the sky block and before emission; each traced ray counts into the pass's ray count
 * SWAP IDENTITY: a scene whose UBO light has intensity 0 and whose list is [L] produces the bits of the same scene under UBO light L with an
 * empty list, in each of the three passes.
 * Shadows and AO do not shade hits and do not change.  hr_ddgi_trace_stats and hr_reflections_trace_stats (and the divergence build) have no
 * instantiation with a list: HR_ERR_UNSUPPORTED on a scene with a non-empty list, before anything is enqueued.
 */

/* The list is host state, read when a pass enqueues (like hr_scene_set_emission); every kind of scene (flat, private-copy instanced, shared,
 * deformable).  The device table of HR_MAX_LIGHTS records is allocated by the first call of either setter (not under stream capture), never after.
 * 0 <= n <= HR_MAX_LIGHTS; n == 0 clears the list (host_lights may then be NULL): off.  Each light is checked — every component finite,
 * data3[0] in {0, 1, 2}, intensity data0[3] >= 0, radius data1[3] >= 0 — and a violation is HR_ERR_INVALID_ARG with hr_last_error naming the
 * index; nothing changes then.  Copied before the call returns; ordered on `stream`; not capturable. */
hr_status hr_scene_set_lights(hr_scene* scene, const hr_light* host_lights, int32_t n, void* stream);
/* dev_lights: DEVICE, the same n records as the last host call set (n == 0: nothing to copy).  One device copy on `stream`: capturable after
 * the first setter call, and UNCHECKED — the values are the caller's responsibility.  hr_scene_get_lights keeps returning the host's list. */
hr_status hr_scene_set_lights_device(hr_scene* scene, const hr_light* dev_lights, void* stream);
/* What the host last set.  host_out: room for HR_MAX_LIGHTS records, or NULL to ask for the count alone. */
hr_status hr_scene_get_lights(const hr_scene* scene, hr_light* host_out, int32_t* n);

/* ---- the primary surfaces: hr_lights --------------------------------------------------------------------------------------------------------
 * Full resolution, in the composite's space.  Per surface texel: albedo, metallic, roughness, P, N, Wo, F0 and the diffuse colour are decoded
 * with the composite's operations (deferred.frag:177-205 as hr_deferred_render performs them); for each light of the scene's list, in list
 * order, fetch_light_properties without SOFT_SHADOWS; where attenuation > 0 one any-hit ray from P + N * bias over [0.01, t_max), of class
 * HR_RAY_SHADOW, through the cutout view; vis = occluded ? 0 : 1 (1 where no ray is traced);
 *   term = (((1 * brdf) * attenuation) * Li) * vis       the composite's own expression, with vis where the shadow image was
 * The sum starts at +0 and runs in list order.  Output RGBA16F, tightly pitched: (fp16 sum, 1) on a surface texel, (0, 0, 0, 0) where
 * depth == 1.  With an empty list every surface texel is (0, 0, 0, 1).
 * hr_deferred_add_emissive (hr_emission.h) adds any RGBA16F image after the composite: this pass's image too. */
typedef struct hr_lights hr_lights;
typedef struct
{
    float bias;   /* hr_shadows' default: 0.5 */
} hr_lights_params;

void      hr_lights_default_params(hr_lights_params* p);
hr_status hr_lights_create(hr_ctx* ctx, int32_t width, int32_t height, hr_lights** out);
hr_status hr_lights_destroy(hr_lights* p);
/* reads in->cur_full when it is set, else in->cur (gb1, gb2, gb3, depth of the pass's extent) and in->ubo's view_proj_inverse and cam_pos */
hr_status hr_lights_render(hr_lights* p, const hr_scene* scene, const hr_frame_inputs* in, const hr_lights_params* params, void* stream);
hr_status hr_lights_output(hr_lights* p, hr_image_view* out);

#ifdef __cplusplus
}
#endif
#endif
