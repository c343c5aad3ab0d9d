/* hr_env_sources.h — what fills an hr_env's sky on the GPU (replaces dw::EquirectangularToCubemap over the Radiance .hdr maps,
 * common.cpp:597-612, and the procedural sky re-rendered when the light moves, main.cpp:980), C ABI.
 *
 * Both update calls write the env's own sky storage ([6][S][S] RGBA16F; the pointers hr_env_get hands out do not change), then enqueue what
 * hr_env_update enqueues behind its copy — the same SH9 and prefilter launches — on the caller's stream: no host synchronisation, no
 * allocation, capturable into a hipGraph.  The one exception is the first hr_env_update_equirect on an env (contract 1).  Calls on one
 * hr_env are externally serialised, as in hr_env.h.
 *
 * Library: hybrid_rendering_amd/libhybrid_rendering_amd.so (csrc/env_sources.hip).  As in hr_env.h, every fp32 operation below is one
 * correctly rounded operation, nothing is contracted, sums are taken in the order written; dot3, normalize3, the texel direction and the
 * face table are hr_env.h's.
 */
#ifndef HR_ENV_SOURCES_H
#define HR_ENV_SOURCES_H

#include "hr_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- contract 1: equirect to cubemap ---------------------------------------------------------------------------------------------------
 * Table (host, double precision, once per hr_env: the first hr_env_update_equirect allocates 6*S*S*8 bytes and uploads them synchronously;
 * it refuses a capturing stream with HR_ERR_INVALID_ARG; later calls may be captured; sky_size > 1024: HR_ERR_UNSUPPORTED).
 *   Face f, texel (x, y):  a = 2*((x + 0.5)/S) - 1, b likewise from y;  d = hr_env.h's face direction with u = a, v = b;
 *   u = atan2(d.z, d.x)/(2*pi) + 0.5;  v = acos(d.y/|d|)/pi;  entry = ((float)u, (float)v).  hr_env_equirect_table returns these floats.
 * Kernel (fp32, one lane per cube texel), over the image [h][w][4] fp32 (alpha is not read), row 0 = the +Y pole:
 *   X = u*w - 0.5;  x0 = floor(X);  fx = X - x0;  columns x0 and x0 + 1 modulo w (longitude wraps).
 *   Y = v*h - 0.5;  y0 = floor(Y);  fy = Y - y0;  rows y0 and y0 + 1 clamped to [0, h - 1].
 *   per channel of rgb:  top = p00*(1 - fx) + p01*fx;  bot = p10*(1 - fx) + p11*fx;  c = top*(1 - fy) + bot*fy.
 *   Stored:  c > 0 ? min(c, 65504) : 0  (a NaN becomes 0), fp16 round to nearest even; alpha = 1.
 * The source is sampled bilinearly at one point per cube texel, as the reference's converter does: a map much larger than 4*S x 2*S aliases.
 *
 * ---- contract 2: analytic sky (after Preetham, Shirley and Smits 1999; the constants here are the specification) ------------------------
 * Host, double, per call -> 24 floats in the kernel's arguments (hr_sky_coefficients returns the same 24):
 *   s = sun_dir/|sun_dir|;  ths = acos(clamp(s.y, 0, 1));  T = turbidity.   Perez coefficients (A, B, C, D, E):
 *   Y: 0.1787T - 1.4630, -0.3554T + 0.4275, -0.0227T + 5.3251,  0.1206T - 2.5771, -0.0670T + 0.3703
 *   x: -0.0193T - 0.2592, -0.0665T + 0.0008, -0.0004T + 0.2125, -0.0641T - 0.8989, -0.0033T + 0.0452
 *   y: -0.0167T - 0.2608, -0.0950T + 0.0092, -0.0079T + 0.2102, -0.0441T - 1.6537, -0.0109T + 0.0529
 *   chi = (4/9 - T/120)(pi - 2 ths);  Yz = (4.0453T - 4.9710) tan(chi) - 0.2155T + 2.4192;
 *   xz = [T^2 T 1] Mx [ths^3 ths^2 ths 1]^T,  Mx = ((0.00166, -0.00375, 0.00209, 0), (-0.02903, 0.06377, -0.03202, 0.00394),
 *   (0.11693, -0.21196, 0.06052, 0.25886));  yz likewise,  My = ((0.00275, -0.00610, 0.00317, 0), (-0.04214, 0.08970, -0.04153, 0.00516),
 *   (0.15346, -0.26756, 0.06670, 0.26688)).
 *   F(th, g) = (1 + A exp(B/cos th)) (1 + C exp(D g) + E cos^2 g);  k_q = zenith_q / F_q(0, ths)  for q in Y, x, y.
 *   out = the 15 coefficients (Y, x, y, each A..E), kY, kx, ky, s.xyz, scale, ground_albedo[0..1]; ground_albedo[2] is its own argument.
 * Kernel (fp32, one lane per cube texel), N = normalize3(texel direction):
 *   ct = max(N.y, 0.02f);  cg = clamp(dot3(N, s), -1, 1);  g = acosf(cg);
 *   q = (k_q*(1 + A_q*expf(B_q/ct))) * ((1 + C_q*expf(D_q*g)) + (E_q*cg)*cg)  for q in Y, x, y;
 *   X = (x/y)*Y;  Z = (((1 - x) - y)/y)*Y;   R = (3.2404542f*X - 1.5371385f*Y) - 0.4985314f*Z;
 *   G = (-0.9692660f*X + 1.8760108f*Y) + 0.0415560f*Z;   B = (0.0556434f*X - 0.2040259f*Y) + 1.0572252f*Z;
 *   rgb *= scale, and rgb *= ground_albedo where N.y < 0;  stored as in contract 1.
 * expf and acosf are the device library's: this path is held to a tolerance (tests/test_gpu_env_sources.py), contract 1 to the bit.
 */

/* equirect_device: [h][w][4] fp32 in device memory, 1 <= w, h <= 16384. */
hr_status hr_env_update_equirect(hr_env* env, const float* equirect_device, int32_t w, int32_t h, void* stream);

typedef struct
{
    float sun_dir[3];       /* towards the sun; any finite non-zero length */
    float turbidity;        /* 1.7 .. 10 */
    float scale;            /* >= 0: multiplies the rgb */
    float ground_albedo[3]; /* >= 0: multiplies the rgb of texels below the horizon */
} hr_sky_params;            /* 32 bytes */

void      hr_sky_default_params(hr_sky_params* p); /* (0.3, 0.9, 0.2), 2.5, 0.1, (0.2, 0.2, 0.2) */
/* The parameters are read by this call: a captured update replays the sky of the capture. */
hr_status hr_env_update_sky(hr_env* env, const hr_sky_params* p, void* stream);
/* Host only, no device is needed: the table of contract 1, host_out = [6][s][s][2] floats (s: a power of two in 4..1024; 2048: HR_ERR_UNSUPPORTED), and
 * the 24 floats of contract 2 (the parameters are checked as hr_env_update_sky checks them). */
hr_status hr_env_equirect_table(int32_t sky_size, float* host_out);
hr_status hr_sky_coefficients(const hr_sky_params* p, float out[24]);
/* Stages env_equirect / env_sky (hr_env_get_stage_times), in front of env_sh9 and env_prefilter. */

#ifdef __cplusplus
}
#endif
#endif
