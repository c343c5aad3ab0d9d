// C++ host shim over include/hr_env.h, in the manner of passes.hpp: what CommonResources::sky_environment holds behind the sky render
// (common.h:91-103: cubemap_sh_projection, cubemap_prefilter) plus brdf_preintegrate_lut (common.h:228), as one object.
//
//   reference (main.cpp:975-990, a frame in which the sun moved)     this header
//   ---------------------------------------------------------------  ---------------------------------------------------------------
//   hosek_wilkie_sky_model->update(cmd_buf, sun_dir)                 the application renders its sky into a device buffer
//                                                                    ... or env.update_sky(cmd_buf, params) / env.update_equirect(cmd_buf, ...)
//   cubemap_sh_projection->update(cmd_buf)                           env.update(cmd_buf, sky)      (both, and the copy of the sky)
//   cubemap_prefilter->update(cmd_buf)
//   write_descriptor_sets(...)                                       nothing: the pointers env.get() hands out never change
//
// common.environment = &env.get() once; deferred.bind(env) once (or env.bind_sh9(deferred.handle())).
#pragma once
#include "../hr_env_sources.h"
#include "passes.hpp"

namespace hr {

class Environment
{
public:
    static hr_env_desc default_desc()
    {
        hr_env_desc d;
        hr_env_default_desc(&d);
        return d;
    }
    explicit Environment(Context& ctx) : Environment(ctx, default_desc()) {}
    Environment(Context& ctx, const hr_env_desc& desc) : m_desc(desc)
    {
        check(hr_env_create(ctx.handle(), &desc, &m_env), "hr_env_create");
        check(hr_env_get(m_env, &m_environment), "hr_env_get");
        check(hr_env_sh9_device(m_env, &m_sh9), "hr_env_sh9_device");
    }
    ~Environment() { hr_env_destroy(m_env); }
    Environment(const Environment&) = delete;
    Environment& operator=(const Environment&) = delete;

    // sky: device [6][sky_size][sky_size] RGBA16F.  Enqueues the copy and the SH9 / prefilter launches on cmd_buf; no host work
    void update(Stream cmd_buf, const void* sky) { check(hr_env_update(m_env, sky, cmd_buf), "Environment::update"); }
    // hr_env_sources.h: the sky from an equirectangular map, device [h][w][4] fp32 (the first call on an env allocates and must not be captured),
    // or from the analytic model; then the same launches as update.  The parameters are read by the call: a captured update_sky replays them
    void update_equirect(Stream cmd_buf, const float* equirect, int32_t w, int32_t h) { check(hr_env_update_equirect(m_env, equirect, w, h, cmd_buf), "Environment::update_equirect"); }
    void update_sky(Stream cmd_buf, const hr_sky_params& params) { check(hr_env_update_sky(m_env, &params, cmd_buf), "Environment::update_sky"); }
    // what Frame::environment / CommonResources::environment point to; valid for the life of this object
    const hr_environment& get() const { return m_environment; }
    const float*          sh9_device() const { return m_sh9; }
    // the composite reads SH9 from this object's device memory from now on (nullptr to hr_deferred_bind_sh9 undoes it)
    void bind_sh9(hr_deferred* deferred) const { check(hr_deferred_bind_sh9(deferred, m_sh9), "hr_deferred_bind_sh9"); }
    void read_sh9(float out[9][4]) { check(hr_env_read_sh9(m_env, out), "hr_env_read_sh9"); }
    void set_profiling(bool on) { check(hr_env_set_profiling(m_env, on ? 1 : 0), "hr_env_set_profiling"); }
    hr_stage_times stage_times()
    {
        hr_stage_times t;
        check(hr_env_get_stage_times(m_env, &t), "hr_env_get_stage_times");
        return t;
    }
    const hr_env_desc& desc() const { return m_desc; }
    hr_env*            handle() const { return m_env; }

private:
    hr_env_desc    m_desc;
    hr_env*        m_env = nullptr;
    hr_environment m_environment;
    const float*   m_sh9 = nullptr;
};

} // namespace hr
