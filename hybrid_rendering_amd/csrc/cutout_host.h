// Host side of cutout.h: the view a CUTOUT launch passes to its walks.
#pragma once
#include "hr_internal.h"
#include "cutout.h"

namespace hr {

// only meaningful while the scene's cutouts are enabled (cutout_on, hr_internal.h): the setter has then allocated and filled cutout_tab
inline CutoutView cutout_view_of(const hr_scene* s)
{
    CutoutView c;
    c.tab       = (const uint2*)s->cutout_tab.p;
    c.uvs       = (const float*)(s->n_instances > 0 ? s->mesh_uvs.p : s->tri_uvs.p);
    c.tex_table = (const uint4*)s->tex_table.p;
    c.tex_data  = (const uint32_t*)s->tex_data.p;
    return c;
}

} // namespace hr
