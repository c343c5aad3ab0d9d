// Host side of lights.h: the view a LIGHTS launch passes to its hit shader.
#pragma once
#include "hr_internal.h"
#include "emission_host.h"
#include "lights.h"

namespace hr {

// only meaningful while lights_live(scene) (hr_internal.h): hr_scene_set_lights has then allocated and filled the table
inline LightsView lights_view_of(const hr_scene* s)
{
    LightsView v;
    v.table = (const hr_light*)s->lights_dev.p;
    v.n     = (int)s->lights_host.size();
    return v;
}

// The LIGHTS instantiations carry emission too (one kernel per pass, not two): a scene whose emission is not live gets a view without
// materials, for which emission_at returns false before it reads anything — no add, as in the kernels without EMISSIVE.
inline EmissionView emission_view_or_none(const hr_scene* s)
{
    if (emission_live(s)) return emission_view_of(s);
    EmissionView e;
    e.rgb = nullptr; e.tex = nullptr; e.n_materials = 0; e.scale = 0.0f;
    return e;
}

} // namespace hr
