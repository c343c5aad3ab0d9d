// The primary ray through a point of the image plane, shared by every kernel that has to agree with the G-buffer's rays (k_gbuffer_raycast,
// api.hip; k_probe_vis, probe_vis.hip): the far-plane point of (px / w, py / h) unprojected, minus the camera position, normalised.
// `a` is any argument block with vpi[16] (column-major view_proj_inverse), cam[3], w and h.
#pragma once
#include "device_math.h"

namespace hr {

template <class Args>
HR_DEV f3 gb_pixel_dir(const Args& a, float px, float py)
{
    f3 far_p = world_pos_from_depth(__fdiv_rn(px, (float)a.w), __fdiv_rn(py, (float)a.h), 1.0f, a.vpi);
    return normalize3(sub3(far_p, mk3(a.cam[0], a.cam[1], a.cam[2])));
}

} // namespace hr
