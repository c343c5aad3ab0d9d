// ORACLE — TEST INFRASTRUCTURE ONLY (see orc_math.h header).  Pinned against the reference's own shaders: tests/test_ref_shaders.py.
// Restatement of the ground-truth path tracer:
//   ground_truth/ground_truth_path_trace.rgen:52-112  primary ray with RNG jitter, running mean in RGBA16F
//   ground_truth/ground_truth_path_trace.rchit:114-142 direct lighting at the first hit: punctual light with
//       SOFT_SHADOWS + sky light (lighting.glsl:117-196 with SOFT_SHADOWS | RAY_THROUGHPUT | SAMPLE_SKY_LIGHT)
//   ground_truth/ground_truth_path_trace.rmiss:24-32  sky cubemap
// indirect_lighting (rchit:67-108) only consumes random numbers and returns p_IndirectPayload.L = 0 because the
// recursive traceRayEXT is commented out (rchit:95-105); nothing reads the RNG afterwards, so it is omitted here.
// Pinned: function arguments are evaluated left to right (rng1 = the two floats after the pixel jitter, rng2 = the next
// two); the sky cubemap is fetched nearest.
#include "orc_api.h"
#include "orc_shading.h"

using namespace orc;

namespace orc {
void fetch_light_properties_shadow(const Light& light, vec3 P, vec3 N, float rx, float ry, vec3* Wi, float* t_max, float* attenuation); // orc_shadows.cpp
}

extern "C" {

// sample_specular_ggx_lobe (brdf.glsl:96-112): orc_shading.h

// prev / cur: [h][w][4] fp16 bit patterns.  rows [y0, y1) are rendered.
// trace_indirect = 0 is the reference as shipped (the recursive traceRayEXT of rchit:95-105 is commented out, so
// indirect_lighting only draws random numbers and returns 0).  trace_indirect = 1 is SURVEY.md section 8f row 3's optional
// extension: that call re-enabled — rchit:67-108 verbatim, including its quirks (sample_uber_brdf takes the RNG BY VALUE, so
// the lobe sample re-uses the numbers the Russian roulette and the next bounce draw; throughput (T * brdf * cos) / pdf).
// Checked against the reference's shaders with those lines un-commented (tests/test_ref_shaders.py).
void orc_ground_truth_render_ex(const void* scene_, const void* ubo_, const uint16_t* sky, int sky_size, int w, int h, int y0, int y1, uint32_t num_frames,
                                float roughness_multiplier, int max_ray_bounces, int trace_indirect, const uint16_t* prev, uint16_t* cur,
                                uint64_t* rays_out)
{
    const Scene& scene = *(const Scene*)scene_;
    const UBO&   ubo   = *(const UBO*)ubo_;
    CubeH        cube { sky, sky_size };
    uint64_t     rays = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : rays)
    for (int y = y0; y < y1; y++)
        for (int x = 0; x < w; x++)
        {
            RNG rng = rng_init((uint32_t)x, (uint32_t)y, num_frames);
            const float jx = next_float(rng), jy = next_float(rng);
            const float px = ((float)x + 0.5f) + jx, py = ((float)y + 0.5f) + jy;
            const float tx = (px / (float)w) * 2.0f - 1.0f, ty = (py / (float)h) * 2.0f - 1.0f;
            const vec4  origin = mul(ubo.view_inverse, vec4 { 0.0f, 0.0f, 0.0f, 1.0f });
            const vec4  target = mul(ubo.proj_inverse, vec4 { tx, ty, 1.0f, 1.0f });
            const vec3  tn     = normalize(v3(target.x, target.y, target.z));
            const vec4  dir4   = mul(ubo.view_inverse, vec4 { tn.x, tn.y, tn.z, 0.0f });
            vec3  o = v3(origin.x, origin.y, origin.z), d = v3(dir4.x, dir4.y, dir4.z);
            // the payload chain of the recursive shader, unrolled: every nested invocation starts with L = 0 and its L is
            // ADDED to its caller's, so the pixel's L is the sum of what each invocation adds, innermost first
            vec3  T = v3(1.0f, 1.0f, 1.0f);
            float t_min = 0.001f;
            vec3  adds[32];
            int   depth = 0;
            for (;; depth++)
            {
                adds[depth] = v3(0, 0, 0);
                rays++;
                const Hit hit = scene.closest_hit(o, d, t_min, 10000.0f);
                if (hit.prim < 0)
                {
                    const vec3 env = cube.fetch(d);
                    adds[depth] = depth == 0 ? env : T * env;   // rmiss:26-34
                    break;
                }
                SurfaceHit sh = surface_at(scene, hit);
                sh.N = normalize(sh.N);   // rchit:131 normalises fetch_normal()'s result once more (observable with normal maps)
                const float roughness = sh.roughness * roughness_multiplier;
                const vec3  Wo = -d;
                const vec3  F0 = mix3(v3(0.04f, 0.04f, 0.04f), sh.albedo, sh.metallic);
                const vec3  c_diffuse = mix3(sh.albedo * (v3(1.0f, 1.0f, 1.0f) - F0), v3(0, 0, 0), sh.metallic);
                const float r1x = next_float(rng), r1y = next_float(rng), r2x = next_float(rng), r2y = next_float(rng);
                vec3        Lo = v3(0, 0, 0);
                const vec3  ray_origin = sh.P + sh.N * 0.1f;
                {
                    vec3  Wi;
                    float t_max, attenuation;
                    fetch_light_properties_shadow(ubo.light, sh.P, sh.N, r1x, r1y, &Wi, &t_max, &attenuation);
                    const vec3 Li = v3(ubo.light.data2[0], ubo.light.data2[1], ubo.light.data2[2]) * ubo.light.data0[3];
                    const vec3 Wh = normalize(Wo + Wi);
                    if (attenuation > 0.0f)
                    {
                        rays++;
                        attenuation = attenuation * (scene.any_hit(ray_origin, Wi, 0.01f, t_max) ? 0.0f : 1.0f);
                    }
                    const vec3 brdf = evaluate_uber_brdf(c_diffuse, roughness, sh.N, F0, Wo, Wh, Wi);
                    Lo = Lo + ((T * brdf) * attenuation) * Li;
                }
                {
                    const vec3 Wi = sample_cosine_lobe(sh.N, r2x, r2y);
                    vec3       Li = cube.fetch(Wi);
                    const vec3 Wh = normalize(Wo + Wi);
                    rays++;
                    Li = Li * (scene.any_hit(ray_origin, Wi, 0.01f, 10000.0f) ? 0.0f : 1.0f);
                    const vec3 brdf = evaluate_uber_brdf(c_diffuse, roughness, sh.N, F0, Wo, Wh, Wi);
                    Lo = Lo + (T * brdf) * Li;
                }
                adds[depth] = Lo;   // p_Payload.L += direct_lighting(...) on a payload whose L is still 0
                if (!trace_indirect || !((uint32_t)(depth + 1) < (uint32_t)max_ray_bounces) || depth + 1 >= 31) break;
                // indirect_lighting (rchit:67-108)
                RNG   copy = rng;                                       // `in RNG rng`: by value
                const float rvx = next_float(copy), rvy = next_float(copy), rvz = next_float(copy);
                const float alpha = roughness * roughness;
                vec3 Wi, Wh;
                if (rvx < 0.5f)
                {
                    Wh = sample_specular_ggx_lobe(sh.N, alpha, rvy, rvz);
                    const vec3 I = -Wo;
                    Wi = roughness < 0.05f ? I - sh.N * (2.0f * dot(sh.N, I)) : I - Wh * (2.0f * dot(Wh, I));
                }
                else
                {
                    Wi = sample_cosine_lobe(sh.N, rvy, rvz);
                    Wh = normalize(Wo + Wi);
                }
                const float NdotL = glsl_max(dot(sh.N, Wi), 0.0f), NdotH = glsl_max(dot(sh.N, Wh), 0.0f), VdotH = glsl_max(dot(Wi, Wh), 0.0f);
                const float pd  = NdotL / ORC_M_PI;
                const float ps  = (D_ggx(NdotH, alpha) * NdotH) / glsl_max(ORC_EPSILON, 4.0f * VdotH);
                const float pdf = mixf(pd, ps, 0.5f);
                const vec3  brdf = evaluate_uber_brdf(c_diffuse, roughness, sh.N, F0, Wo, Wh, Wi);
                const float cos_theta = glsl_clamp(dot(sh.N, Wi), 0.0f, 1.0f);
                vec3 Tn = (T * (brdf * cos_theta)) / pdf;
                const float probability = glsl_max(Tn.x, glsl_max(Tn.y, Tn.z));
                if (next_float(rng) > probability) break;
                Tn = Tn * (1.0f / probability);
                T = Tn; o = sh.P; d = Wi; t_min = 0.0001f;
            }
            // unwind: L_k = adds[k] + L_{k+1}
            vec3 L = adds[depth];
            for (int k = depth - 1; k >= 0; k--) L = adds[k] + L;
            const vec3 clamped = v3(glsl_min(L.x, 1.0f), glsl_min(L.y, 1.0f), glsl_min(L.z, 1.0f)); // RADIANCE_CLAMP_COLOR (common.glsl:19)
            vec3 out = clamped;
            const size_t o4 = ((size_t)y * w + x) * 4;
            if (num_frames != 0)
            {
                const vec3 pc = v3(f16_to_f32(prev[o4 + 0]), f16_to_f32(prev[o4 + 1]), f16_to_f32(prev[o4 + 2]));
                const float n = (float)num_frames;
                out = v3(pc.x + (clamped.x - pc.x) / n, pc.y + (clamped.y - pc.y) / n, pc.z + (clamped.z - pc.z) / n);
            }
            cur[o4 + 0] = f32_to_f16(out.x); cur[o4 + 1] = f32_to_f16(out.y); cur[o4 + 2] = f32_to_f16(out.z); cur[o4 + 3] = f32_to_f16(1.0f);
        }
    if (rays_out) *rays_out = rays;
}

void orc_ground_truth_render(const void* scene_, const void* ubo_, const uint16_t* sky, int sky_size, int w, int h, int y0, int y1, uint32_t num_frames,
                             float roughness_multiplier, const uint16_t* prev, uint16_t* cur, uint64_t* rays_out)
{
    orc_ground_truth_render_ex(scene_, ubo_, sky, sky_size, w, h, y0, y1, num_frames, roughness_multiplier, 2, 0, prev, cur, rays_out);
}

} // extern "C"
