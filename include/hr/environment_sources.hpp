// C++ host shim over include/hr_env_sources.h: the two sources of an hr::Environment's sky and their host-only helpers.
//
//   reference                                                          this header
//   -----------------------------------------------------------------  -------------------------------------------------------------
//   dw::EquirectangularToCubemap::convert(hdr image, cubemap)            env.update_equirect(cmd_buf, device fp32 [h][w][4], w, h)
//     (common.cpp:597-612, once per .hdr map)                             (then SH9 and the prefiltered chain, as env.update does)
//   sky model ->update(cmd_buf, sun_dir)   (main.cpp:980)                env.update_sky(cmd_buf, hr::SkyParams().sun(x, y, z))
//
// hr::Environment::update_equirect / update_sky themselves are members of hr::Environment (environment.hpp).
#pragma once
#include "environment.hpp"
#include <vector>

namespace hr {

// hr_sky_params with hr_sky_default_params' values, and setters that chain
struct SkyParams : hr_sky_params
{
    SkyParams() { hr_sky_default_params(this); }
    SkyParams& sun(float x, float y, float z) { sun_dir[0] = x; sun_dir[1] = y; sun_dir[2] = z; return *this; }
    SkyParams& set_turbidity(float t) { turbidity = t; return *this; }
    SkyParams& set_scale(float s) { scale = s; return *this; }
    SkyParams& ground(float r, float g, float b) { ground_albedo[0] = r; ground_albedo[1] = g; ground_albedo[2] = b; return *this; }
};

// host only: the (u, v) of every cube texel, [6][sky_size][sky_size][2], and the 24 floats the sky kernel takes
inline std::vector<float> equirect_table(int32_t sky_size)
{
    std::vector<float> t(sky_size > 0 ? (size_t)12 * sky_size * sky_size : 0);
    check(hr_env_equirect_table(sky_size, t.data()), "hr_env_equirect_table");
    return t;
}
inline std::vector<float> sky_coefficients(const hr_sky_params& p)
{
    std::vector<float> c(24);
    check(hr_sky_coefficients(&p, c.data()), "hr_sky_coefficients");
    return c;
}

} // namespace hr
