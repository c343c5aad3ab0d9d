// C++ host shim over include/hr_emission.h, in the manner of passes.hpp: emissive materials.  (The reference defines fetch_emissive and calls it
// from no shader: there is no class to mirror.)  Free functions over the classes of passes.hpp.
//
//   a frame with emissive surfaces, everything on one stream (cmd_buf)
//   ----------------------------------------------------------------------------------------------------------------------------------------
//   once:       hr::set_emission(scene, true, 1.0f, cmd_buf);   hr::set_emissive_textures(scene, tex, cmd_buf);
//   per frame:  hr::set_emissive(scene, rgb, cmd_buf);                           // blinking, dimming; or set_emissive_device (capturable)
//               the passes — DDGI, reflections and the ground truth add E at their hits
//               deferred.render(...);
//               hr::gbuffer_emissive(scene, ubo, w, h, image_device, cmd_buf);   // or the integrator's own image from its raster G-buffer
//               hr::add_emissive(deferred, image_view, cmd_buf);                 // before TAA
#pragma once
#include "../hr_emission.h"
#include "passes.hpp"

namespace hr {

inline void set_emission(Scene& scene, bool enable, float scale = 1.0f, Stream cmd_buf = nullptr)
{
    check(hr_scene_set_emission(scene.handle(), enable ? 1 : 0, scale, cmd_buf), "hr_scene_set_emission");
}
inline bool emission_enabled(const Scene& scene, float* scale = nullptr)
{
    int32_t on = 0;
    check(hr_scene_get_emission(scene.handle(), &on, scale), "hr_scene_get_emission");
    return on != 0;
}
// host [n_materials][3], finite and >= 0
inline void set_emissive(Scene& scene, const float* rgb, Stream cmd_buf = nullptr) { check(hr_scene_set_emissive(scene.handle(), rgb, cmd_buf), "hr_scene_set_emissive"); }
// device [n_materials][3]: one device copy, capturable, unchecked
inline void set_emissive_device(Scene& scene, const float* rgb_device, Stream cmd_buf = nullptr)
{
    check(hr_scene_set_emissive_device(scene.handle(), rgb_device, cmd_buf), "hr_scene_set_emissive_device");
}
// host [n_materials]: indices into the scene's textures, -1 = none
inline void set_emissive_textures(Scene& scene, const int32_t* tex, Stream cmd_buf = nullptr)
{
    check(hr_scene_set_emissive_textures(scene.handle(), tex, cmd_buf), "hr_scene_set_emissive_textures");
}
// E of n hits as hr_trace_closest_hit reports them; out: device [n][3] fp32
inline void emission(const Scene& scene, int64_t n, const int32_t* prim_device, const float* tuv_device, float* out_device, Stream cmd_buf = nullptr)
{
    check(hr_scene_emission(scene.handle(), n, prim_device, tuv_device, out_device, cmd_buf), "hr_scene_emission");
}
// the emissive image of the primary hits; out: device RGBA16F [height][width]
inline void gbuffer_emissive(const Scene& scene, const hr_ubo& ubo, int32_t width, int32_t height, void* out_device, Stream cmd_buf = nullptr)
{
    check(hr_gbuffer_emissive(scene.handle(), &ubo, width, height, out_device, cmd_buf), "hr_gbuffer_emissive");
}
// colour.rgb += emissive.rgb on the composite's output, after DeferredShading::render on the same stream and before TAA
inline void add_emissive(DeferredShading& deferred, const hr_image_view& emissive, Stream cmd_buf = nullptr)
{
    check(hr_deferred_add_emissive(deferred.handle(), &emissive, cmd_buf), "hr_deferred_add_emissive");
}

} // namespace hr
