// Host side of emission.h: the view an EMISSIVE launch passes to its hit shader.
#pragma once
#include "hr_internal.h"
#include "emission.h"

namespace hr {

// only meaningful while emission_live(scene) (hr_internal.h): hr_scene_set_emission has then allocated and filled the tables
inline EmissionView emission_view_of(const hr_scene* s)
{
    EmissionView e;
    e.rgb         = (const float*)s->em_rgb.p;
    e.tex         = (const int32_t*)s->em_tex.p;
    e.n_materials = s->n_materials;
    e.scale       = s->emission_scale;
    return e;
}

} // namespace hr
