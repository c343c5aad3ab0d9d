// What fills an hr_env's sky on MI355X — HIP replacement for the two ways the reference makes its sky cubemap, both framework classes outside
// its tree: dw::EquirectangularToCubemap over the Radiance .hdr maps (common.cpp:597-612) and the procedural sky re-rendered when the light
// moves (main.cpp:980, common.cpp:543).  The arithmetic is specified in include/hr_env_sources.h and restated in numpy by
// tests/env_sources_reference.py; both kernels follow that text operation by operation.  Behind either kernel runs env.hip's
// env_enqueue_derived: the launches hr_env_update enqueues behind its copy.
#include "env_internal.h"
#include "../../include/hr_env_sources.h"
#include <cmath>

using namespace hr;

namespace hr { bool stream_is_capturing(hipStream_t st); }   // instances_shared_update.hip

namespace {

constexpr int    kMaxTableSky = 1024, kMaxSkySize = 2048, kMaxEquirect = 16384;
constexpr double kPi = 3.14159265358979323846;

struct SkyCoef { float v[24]; };   // hr_env_sources.h contract 2 "out"

// contract 1 and 2 "Stored": NaN and everything <= 0 become +0, the rest saturates at the largest finite fp16
HR_DEV float stored(float c) { return c > 0.0f ? (c < 65504.0f ? c : 65504.0f) : 0.0f; }

// contract 1 "Kernel": one lane per cube texel
__global__ __launch_bounds__(256) void k_env_equirect(const float2* __restrict__ table, const float* __restrict__ img, int w, int h, long long texels,
                                                      uint2* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= texels) return;
    const float2 uv = table[t];
    const float X = uv.x * (float)w - 0.5f, xf = floorf(X), fx = X - xf, gx = 1.0f - fx;
    const float Y = uv.y * (float)h - 0.5f, yf = floorf(Y), fy = Y - yf, gy = 1.0f - fy;
    // x0 is in [-1, w] and y0 in [-1, h - 1] for every table entry; the wrap and the clamp below hold for any int
    const int x0 = (int)xf, y0 = (int)yf;
    int xa = x0 % w, xb = inc_sat(x0) % w;
    xa = xa < 0 ? xa + w : xa;
    xb = xb < 0 ? xb + w : xb;
    const int ya = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0), y1 = inc_sat(y0), yb = y1 < 0 ? 0 : (y1 > h - 1 ? h - 1 : y1);
    const float* __restrict__ p00 = img + ((size_t)ya * w + xa) * 4;
    const float* __restrict__ p01 = img + ((size_t)ya * w + xb) * 4;
    const float* __restrict__ p10 = img + ((size_t)yb * w + xa) * 4;
    const float* __restrict__ p11 = img + ((size_t)yb * w + xb) * 4;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const float top = p00[k] * gx + p01[k] * fx;
        const float bot = p10[k] * gx + p11[k] * fx;
        c[k] = stored(top * gy + bot * fy);
    }
    out[t] = make_uint2(pack_h2(c[0], c[1]), pack_h2(c[2], 1.0f));
}

// contract 2: q = (k*(1 + A*expf(B/ct))) * ((1 + C*expf(D*g)) + (E*cg)*cg);  c = A..E
HR_DEV float perez(const float* c, float k, float ct, float g, float cg)
{
    const float zen = 1.0f + c[0] * expf(__fdiv_rn(c[1], ct));
    const float sun = (1.0f + c[2] * expf(c[3] * g)) + (c[4] * cg) * cg;
    return (k * zen) * sun;
}

// contract 2 "Kernel": one lane per cube texel
__global__ __launch_bounds__(256) void k_env_sky(SkyCoef co, float ground_b, int S, uint2* __restrict__ out)
{
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);   // 6*S*S <= 6 * 2048^2: an int holds it
    if (t >= 6 * S * S) return;
    const int x = t % S, y = (t / S) % S, face = t / (S * S);
    const f3    N  = normalize3(texel_dir(face, x, y, S));
    const float ct = max2(N.y, 0.02f);
    const float cg = clamp1(dot3(N, mk3(co.v[18], co.v[19], co.v[20])), -1.0f, 1.0f);
    const float g  = acosf(cg);
    const float Yl = perez(co.v + 0, co.v[15], ct, g, cg);
    const float cx = perez(co.v + 5, co.v[16], ct, g, cg);
    const float cy = perez(co.v + 10, co.v[17], ct, g, cg);
    const float X  = __fdiv_rn(cx, cy) * Yl;
    const float Z  = __fdiv_rn((1.0f - cx) - cy, cy) * Yl;
    float r = (3.2404542f * X - 1.5371385f * Yl) - 0.4985314f * Z;
    float gr = (-0.9692660f * X + 1.8760108f * Yl) + 0.0415560f * Z;
    float b = (0.0556434f * X - 0.2040259f * Yl) + 1.0572252f * Z;
    const float scale = co.v[21];
    r = r * scale; gr = gr * scale; b = b * scale;
    if (N.y < 0.0f) { r = r * co.v[22]; gr = gr * co.v[23]; b = b * ground_b; }
    out[t] = make_uint2(pack_h2(stored(r), stored(gr)), pack_h2(stored(b), 1.0f));
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

// contract 1 "Table"
void equirect_table(int S, float* out)
{
    for (int f = 0; f < 6; f++)
        for (int y = 0; y < S; y++)
            for (int x = 0; x < S; x++)
            {
                const double a = 2.0 * (((double)x + 0.5) / (double)S) - 1.0, b = 2.0 * (((double)y + 0.5) / (double)S) - 1.0;
                double d[3];
                switch (f)
                {
                case 0: d[0] = 1.0; d[1] = -b; d[2] = -a; break;
                case 1: d[0] = -1.0; d[1] = -b; d[2] = a; break;
                case 2: d[0] = a; d[1] = 1.0; d[2] = b; break;
                case 3: d[0] = a; d[1] = -1.0; d[2] = -b; break;
                case 4: d[0] = a; d[1] = -b; d[2] = 1.0; break;
                default: d[0] = -a; d[1] = -b; d[2] = -1.0; break;
                }
                const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                const double u = std::atan2(d[2], d[0]) / (2.0 * kPi) + 0.5, v = std::acos(d[1] / len) / kPi;
                float* o = out + (((size_t)f * S + y) * S + x) * 2;
                o[0] = (float)u;
                o[1] = (float)v;
            }
}

bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }

// the refusals of hr_env_update_sky / hr_sky_coefficients, by the field at fault
hr_status check_sky_params(const char* call, const hr_sky_params* p)
{
    if (!p) return bad(call, "p is NULL");
    const float* s = p->sun_dir;
    if (!(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2])) || (s[0] == 0.0f && s[1] == 0.0f && s[2] == 0.0f))
        return bad(call, "sun_dir must be finite and non-zero");
    if (!(p->turbidity >= 1.7f && p->turbidity <= 10.0f)) return bad(call, "turbidity outside [1.7, 10]");
    if (!finite_nonneg(p->scale)) return bad(call, "scale must be finite and >= 0");
    if (!(finite_nonneg(p->ground_albedo[0]) && finite_nonneg(p->ground_albedo[1]) && finite_nonneg(p->ground_albedo[2])))
        return bad(call, "ground_albedo must be finite and >= 0");
    return HR_OK;
}

double perez_host(const double* c, double theta, double gamma)
{
    return (1.0 + c[0] * std::exp(c[1] / std::cos(theta))) * (1.0 + c[2] * std::exp(c[3] * gamma) + c[4] * std::cos(gamma) * std::cos(gamma));
}

// contract 2 "Host"
void sky_coefficients(const hr_sky_params* p, float out[24])
{
    const double sx = p->sun_dir[0], sy = p->sun_dir[1], sz = p->sun_dir[2], len = std::sqrt(sx * sx + sy * sy + sz * sz);
    const double s[3] = { sx / len, sy / len, sz / len };
    const double ths = std::acos(s[1] < 0.0 ? 0.0 : (s[1] > 1.0 ? 1.0 : s[1])), T = (double)p->turbidity;
    const double co[3][5] = { { 0.1787 * T - 1.4630, -0.3554 * T + 0.4275, -0.0227 * T + 5.3251, 0.1206 * T - 2.5771, -0.0670 * T + 0.3703 },
                              { -0.0193 * T - 0.2592, -0.0665 * T + 0.0008, -0.0004 * T + 0.2125, -0.0641 * T - 0.8989, -0.0033 * T + 0.0452 },
                              { -0.0167 * T - 0.2608, -0.0950 * T + 0.0092, -0.0079 * T + 0.2102, -0.0441 * T - 1.6537, -0.0109 * T + 0.0529 } };
    static const double Mx[3][4] = { { 0.00166, -0.00375, 0.00209, 0.0 }, { -0.02903, 0.06377, -0.03202, 0.00394 }, { 0.11693, -0.21196, 0.06052, 0.25886 } };
    static const double My[3][4] = { { 0.00275, -0.00610, 0.00317, 0.0 }, { -0.04214, 0.08970, -0.04153, 0.00516 }, { 0.15346, -0.26756, 0.06670, 0.26688 } };
    const double chi = (4.0 / 9.0 - T / 120.0) * (kPi - 2.0 * ths);
    const double tv[3] = { T * T, T, 1.0 }, th[4] = { ths * ths * ths, ths * ths, ths, 1.0 };
    double zen[3] = { (4.0453 * T - 4.9710) * std::tan(chi) - 0.2155 * T + 2.4192, 0.0, 0.0 };
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++)
        {
            zen[1] += tv[i] * Mx[i][j] * th[j];
            zen[2] += tv[i] * My[i][j] * th[j];
        }
    for (int q = 0; q < 3; q++)
    {
        for (int k = 0; k < 5; k++) out[q * 5 + k] = (float)co[q][k];
        out[15 + q] = (float)(zen[q] / perez_host(co[q], 0.0, ths));
        out[18 + q] = (float)s[q];
    }
    out[21] = p->scale;
    out[22] = p->ground_albedo[0];
    out[23] = p->ground_albedo[1];
}

unsigned texel_blocks(int S) { return (unsigned)(((size_t)6 * S * S + 255) / 256); }

} // namespace

extern "C" {

void hr_sky_default_params(hr_sky_params* p)
{
    if (!p) return;
    p->sun_dir[0] = 0.3f; p->sun_dir[1] = 0.9f; p->sun_dir[2] = 0.2f;
    p->turbidity = 2.5f; p->scale = 0.1f;
    p->ground_albedo[0] = p->ground_albedo[1] = p->ground_albedo[2] = 0.2f;
}

hr_status hr_env_equirect_table(int32_t sky_size, float* host_out)
{
    static const char* call = "hr_env_equirect_table";
    if (!host_out) return bad(call, "host_out is NULL");
    if (!(pow2(sky_size) && sky_size >= 4 && sky_size <= kMaxSkySize)) return bad(call, "sky_size must be a power of two in 4..1024");
    if (sky_size > kMaxTableSky)
    {
        set_last_error(std::string(call) + ": sky_size > 1024 is not supported");
        return HR_ERR_UNSUPPORTED;
    }
    equirect_table(sky_size, host_out);
    return HR_OK;
}

hr_status hr_sky_coefficients(const hr_sky_params* p, float out[24])
{
    static const char* call = "hr_sky_coefficients";
    hr_status s = check_sky_params(call, p);
    if (s != HR_OK) return s;
    if (!out) return bad(call, "out is NULL");
    sky_coefficients(p, out);
    return HR_OK;
}

hr_status hr_env_update_equirect(hr_env* e, const float* equirect_device, int32_t w, int32_t h, void* stream)
{
    static const char* call = "hr_env_update_equirect";
    HR_SCOPED_SAMPLE("Environment Update");
    // the image first: its checks need no device
    if (!equirect_device) return bad(call, "equirect_device is NULL");
    if (w < 1 || w > kMaxEquirect) return bad(call, "w outside 1..16384");
    if (h < 1 || h > kMaxEquirect) return bad(call, "h outside 1..16384");
    if (!e) return bad(call, "env is NULL");
    const int S = e->d.sky_size;
    if (S > kMaxTableSky)
    {
        set_last_error(std::string(call) + ": sky_size > 1024 is not supported");
        return HR_ERR_UNSUPPORTED;
    }
    HR_HIP(hipSetDevice(e->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (!e->equirect_table.p)
    {
        if (stream_is_capturing(st))
            return bad(call, "the first call on an env builds and uploads its table: not possible while the stream is capturing (call once before the capture)");
        std::vector<float> host((size_t)6 * S * S * 2);
        equirect_table(S, host.data());
        hr_status s = e->equirect_table.alloc(host.size() * sizeof(float));
        if (s != HR_OK) return s;
        const hipError_t ce = hipMemcpy(e->equirect_table.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
        if (ce != hipSuccess) e->equirect_table.free();   // no half-built table: the next call starts over
        HR_HIP(ce);
    }
    e->prof.begin_frame();
    const int ev = e->prof.begin("env_equirect", st, e->equirect_table.bytes + e->sky.bytes);
    hipLaunchKernelGGL(k_env_equirect, dim3(texel_blocks(S)), dim3(256), 0, st, (const float2*)e->equirect_table.p, equirect_device, (int)w, (int)h,
                       6LL * S * S, (uint2*)e->sky.p);
    e->prof.end(ev, st);
    return env_enqueue_derived(e, st);
}

hr_status hr_env_update_sky(hr_env* e, const hr_sky_params* p, void* stream)
{
    static const char* call = "hr_env_update_sky";
    HR_SCOPED_SAMPLE("Environment Update");
    // the parameters first: their checks need no device
    hr_status s = check_sky_params(call, p);
    if (s != HR_OK) return s;
    if (!e) return bad(call, "env is NULL");
    SkyCoef co;
    sky_coefficients(p, co.v);
    HR_HIP(hipSetDevice(e->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int S = e->d.sky_size;
    e->prof.begin_frame();
    const int ev = e->prof.begin("env_sky", st, e->sky.bytes);
    hipLaunchKernelGGL(k_env_sky, dim3(texel_blocks(S)), dim3(256), 0, st, co, p->ground_albedo[2], S, (uint2*)e->sky.p);
    e->prof.end(ev, st);
    return env_enqueue_derived(e, st);
}

} // extern "C"
