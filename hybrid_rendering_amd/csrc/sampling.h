// The direction samplers of the trace passes, in one place so that hr_selftest_shading (selftest_shading.hip) evaluates the very functions the
// kernels inline: each body is the text that stood in reflections.hip, ground_truth.hip, ao.hip and ddgi.hip.  (EnvDev, which needs CubeMap, and
// sample_cosine_lobe_n are in shading.h.)
#pragma once
#include "device_math.h"

namespace hr {

HR_DEV f3 reflect3(f3 I, f3 N) { return sub3(I, scale3(N, 2.0f * dot3(N, I))); }

// reflections_ray_trace.rgen:78-105
HR_DEV f3 importance_sample_ggx(float Ex, float Ey, f3 N, float roughness)
{
    const float a = roughness * roughness, m2 = a * a;
    const float phi = 2.0f * HR_M_PI * Ex;
    const float ct  = hr_sqrt(__fdiv_rn(1.0f - Ey, 1.0f + (m2 - 1.0f) * Ey));
    const float st  = hr_sqrt(1.0f - ct * ct);
    float s, c;
    det_sincos(phi, s, c);
    const f3 H  = mk3(c * st, s * st, ct);
    const f3 up = fabsf(N.z) < 0.999f ? mk3(0.0f, 0.0f, 1.0f) : mk3(1.0f, 0.0f, 0.0f);
    const f3 tangent   = normalize3(cross3(up, N));
    const f3 bitangent = cross3(N, tangent);
    return normalize3(add3(add3(scale3(tangent, H.x), scale3(bitangent, H.y)), scale3(N, H.z)));
}

// brdf.glsl:96-112 (the ground-truth path tracer's specular bounce)
HR_DEV f3 sample_specular_ggx_lobe(f3 n, float alpha, float xi_x, float xi_y)
{
    const float phi = 2.0f * HR_M_PI * xi_x;
    const float ct  = hr_sqrt(__fdiv_rn(1.0f - xi_y, 1.0f + (alpha * alpha - 1.0f) * xi_y));
    const float st  = hr_sqrt(1.0f - ct * ct);
    float s, c;
    det_sincos(phi, s, c);
    const f3 t   = mk3(st * c, st * s, ct);
    const f3 ref = fabsf(dot3(n, mk3(0.0f, 1.0f, 0.0f))) > 0.99f ? mk3(0.0f, 0.0f, 1.0f) : mk3(0.0f, 1.0f, 0.0f);
    const f3 x   = normalize3(cross3(ref, n));
    const f3 y   = cross3(n, x);
    return normalize3(mk3((x.x * t.x + y.x * t.y) + n.x * t.z, (x.y * t.x + y.y * t.y) + n.y * t.z, (x.z * t.x + y.z * t.y) + n.z * t.z));
}

// brdf.glsl:8-32 sample_cosine_lobe + make_rotation_matrix (the AO trace's; shading.h sample_cosine_lobe_n is the hit shading's, with the
// specification's max where this one keeps max2 — the two differ on a NaN random number only, which no sequence produces)
HR_DEV f3 sample_cosine_lobe(f3 n, float rx, float ry)
{
    rx = max2(0.00001f, rx);
    ry = max2(0.00001f, ry);
    const float phi = 2.0f * HR_M_PI * ry;
    const float ct = hr_sqrt(rx), st = hr_sqrt(1.0f - rx);
    float s, c;
    det_sincos(phi, s, c);
    const f3 t   = mk3(st * c, st * s, ct);
    const f3 ref = fabsf(dot3(n, mk3(0.0f, 1.0f, 0.0f))) > 0.99f ? mk3(0.0f, 0.0f, 1.0f) : mk3(0.0f, 1.0f, 0.0f);
    const f3 x   = normalize3(cross3(ref, n));
    const f3 y   = cross3(n, x);
    return normalize3(mk3((x.x * t.x + y.x * t.y) + n.x * t.z, (x.y * t.x + y.y * t.y) + n.y * t.z, (x.z * t.x + y.z * t.y) + n.z * t.z));
}

// gi_ray_trace.rgen:61-72.  PHI = sqrt(5)*0.5+0.5 evaluated in fp32; PHI - 1 is exact.
HR_DEV f3 spherical_fibonacci(float i, float n)
{
    const float PHI_M1 = 0.61803400516510009765625f;
    const float a   = i * PHI_M1;
    const float phi = 2.0f * HR_M_PI * (a - floorf(a));
    const float ct  = 1.0f - (2.0f * i + 1.0f) * __fdiv_rn(1.0f, n);
    const float st  = hr_sqrt(glsl_clamp(1.0f - ct * ct, 0.0f, 1.0f));
    float s, c;
    det_sincos(phi, s, c);
    return mk3(c * st, s * st, ct);
}

} // namespace hr
