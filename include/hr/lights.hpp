// C++ host shim over include/hr_lights.h, in the manner of passes.hpp: extra lights.  (The reference's UBO carries one Light: there is no class
// to mirror.)  hr::Lights is the primary-surface pass; the list itself is Scene::set_lights (passes.hpp) and the free functions below.
//
//   a frame with a light list, everything on one stream (cmd_buf)
//   ----------------------------------------------------------------------------------------------------------------------------------------
//   once / on change:  scene.set_lights(lights, n, cmd_buf);                       // or hr::set_lights_device (capturable, same n)
//   per frame:         the passes — DDGI, reflections and the ground truth add the list's sum at their hits
//                      deferred.render(...);
//                      lights.render(cmd_buf, frame);                              // hard shadows; soft ones: a second RayTracedShadows under that light
//                      hr::add_lights(deferred, lights.output_ds(), cmd_buf);      // before TAA
// Out of scope: a stage inside HybridFrame, row-band tiling, light culling or a range.
#pragma once
#include "../hr_lights.h"
#include "../hr_emission.h"
#include "passes.hpp"

namespace hr {

// device [n] hr_light, n as the last Scene::set_lights: one device copy, capturable, unchecked
inline void set_lights_device(Scene& scene, const hr_light* lights_device, Stream cmd_buf = nullptr)
{
    check(hr_scene_set_lights_device(scene.handle(), lights_device, cmd_buf), "hr_scene_set_lights_device");
}
// what the host last set; out: room for HR_MAX_LIGHTS records, or nullptr for the count alone
inline int32_t get_lights(const Scene& scene, hr_light* out = nullptr)
{
    int32_t n = 0;
    check(hr_scene_get_lights(scene.handle(), out, &n), "hr_scene_get_lights");
    return n;
}

class Lights
{
public:
    hr_lights_params params;
    Lights(Context& ctx, uint32_t width, uint32_t height)
    {
        hr_lights_default_params(&params);
        check(hr_lights_create(ctx.handle(), (int32_t)width, (int32_t)height, &m_pass), "hr_lights_create");
    }
    ~Lights() { hr_lights_destroy(m_pass); }
    Lights(const Lights&) = delete;
    Lights& operator=(const Lights&) = delete;
    void render(Stream cmd_buf, const Frame& frame) { check(hr_lights_render(m_pass, frame.scene->handle(), &frame.inputs, &params, cmd_buf), "Lights::render"); }
    ImageView output_ds()
    {
        ImageView v;
        check(hr_lights_output(m_pass, &v), "Lights::output_ds");
        return v;
    }
    hr_lights* handle() const { return m_pass; }
private:
    hr_lights* m_pass = nullptr;
};

// colour.rgb += image.rgb on the composite's output (hr_deferred_add_emissive under the lights' name), after DeferredShading::render and before TAA
inline void add_lights(DeferredShading& deferred, const ImageView& image, Stream cmd_buf = nullptr)
{
    check(hr_deferred_add_emissive(deferred.handle(), &image, cmd_buf), "hr_deferred_add_emissive");
}

} // namespace hr
