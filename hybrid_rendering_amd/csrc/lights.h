// Extra lights (contract: include/hr_lights.h): the ONE text of the list's term X in the hit shaders of the LIGHTS trace instantiations
// (ddgi.hip, reflections.hip, ground_truth.hip).  The primary-surface pass (lights.hip) spells its own sum: the composite's expression, not the
// hit shaders'.
#pragma once
#include "shading.h"

namespace hr {

// what the list's loop reads, by value in the kernel arguments of a LIGHTS instantiation (absent from every other).  The table is the scene's
// (hr_scene_set_lights allocates HR_MAX_LIGHTS records); `n` is the host's count.  `k` below is the same in every lane and the table is written
// by no kernel: the record load is wave-uniform (s_load_dwordx16), one per light and wave, not one per lane.
struct LightsView
{
    const hr_light* __restrict__ table;
    int             n;
};

// X = ((+0 + t_0) + t_1) + ... with t_k what direct_lighting's first block (shading.h) adds for its light: fetch_light_hard, one any-hit ray
// where attenuation > 0, ((T * brdf) * attenuation) * Li.  The DDGI and reflection hit shaders.
template <bool CUTOUT, class Ctx>
HR_DEV f3 extra_lights_hard(Ctx& tc, const LightsView& lv, f3 Wo, f3 N, f3 P, f3 F0, f3 diffuse_color, float roughness, f3 T, uint32_t& rays)
{
    f3       X = mk3(0.0f, 0.0f, 0.0f);
    const f3 ray_origin = add3(P, scale3(N, 0.1f));
    uint32_t nn = 0, nt = 0;
    for (int k = 0; k < lv.n; k++)
    {
        const hr_light L = lv.table[k];
        f3    Li, Wi, Wh;
        float t_max, attenuation;
        fetch_light_hard(L, Wo, P, N, Li, Wi, Wh, t_max, attenuation);
        if (attenuation > 0.0f)
        {
            rays++;
            attenuation = attenuation * (visibility_ray_occluded<false, CUTOUT>(tc, ray_origin, Wi, 0.01f, t_max, nn, nt) ? 0.0f : 1.0f);
        }
        const f3 brdf = evaluate_uber_brdf(diffuse_color, roughness, N, F0, Wo, Wh, Wi);
        X = add3(X, mul3(scale3(mul3(T, brdf), attenuation), Li));
    }
    return X;
}

// The ground truth's form: fetch_light_shadow with the two numbers (rx, ry) the UBO light drew at this hit — the list draws nothing.
template <bool CUTOUT, class Ctx>
HR_DEV f3 extra_lights_soft(Ctx& tc, const LightsView& lv, f3 Wo, f3 N, f3 P, f3 ray_origin, f3 F0, f3 diffuse_color, float roughness, f3 T, float rx, float ry, uint32_t& rays)
{
    f3       X = mk3(0.0f, 0.0f, 0.0f);
    uint32_t nn = 0, nt = 0;
    for (int k = 0; k < lv.n; k++)
    {
        const hr_light L = lv.table[k];
        f3    Wi;
        float t_max, attenuation;
        fetch_light_shadow(L, P, N, rx, ry, Wi, t_max, attenuation);
        const f3 Li = scale3(mk3(L.data2[0], L.data2[1], L.data2[2]), L.data0[3]);
        const f3 Wh = normalize3(add3(Wo, Wi));
        if (attenuation > 0.0f)
        {
            rays++;
            attenuation = attenuation * (visibility_ray_occluded<false, CUTOUT>(tc, ray_origin, Wi, 0.01f, t_max, nn, nt) ? 0.0f : 1.0f);
        }
        const f3 brdf = evaluate_uber_brdf(diffuse_color, roughness, N, F0, Wo, Wh, Wi);
        X = add3(X, mul3(scale3(mul3(T, brdf), attenuation), Li));
    }
    return X;
}

} // namespace hr
