// hr_selftest_shading (include/hr_api_post.h): the device shading layer — shading.h, cutout.h, sampling.h — function by function on arrays, so
// that tests/test_gpu_shading_layer.py can compare it bit for bit with the tests' CPU mirror of the same modes at constructed edges a
// scene reaches only by accident.  Test infrastructure: one thread per element, no LDS, no traversal; compiled with the build's default flags, so
// every function is the sequence of individually rounded operations it is inside the kernels.  Every mode calls the product's own function.
#include "hr_internal.h"
#include "shading.h"
#include "selftest_shading.h"
#include <cstring>

using namespace hr;

namespace {

HR_DEV f3 in3(const float* v, int k) { return mk3(v[k], v[k + 1], v[k + 2]); }
HR_DEV void out3(float* r, int k, f3 a) { r[k] = a.x; r[k + 1] = a.y; r[k + 2] = a.z; }
HR_DEV int index_in(float x, int n) { const int i = (int)x; return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }   // a table index from an input float, kept inside the table

HR_DEV void shading_eval(int mode, const float* v, const ShadingTables& T, float* r)
{
    switch (mode)
    {
        case SHADING_RNG:
        {
            Rng g = rng_init(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]));
            for (int k = 0; k < 8; k++) r[k] = next_float(g);
            break;
        }
        case SHADING_CUBE:
        {
            const EnvDev env { CubeMap { T.cube, T.cube_size }, T.prefiltered, T.pre_size, T.pre_levels, T.lut, T.lut_size };
            out3(r, 0, env.sky.fetch(in3(v, 0)));
            out3(r, 3, env.prefiltered_fetch(in3(v, 0), v[3]));
            env.lut_fetch(v[4], v[5], r[6], r[7]);
            break;
        }
        case SHADING_TEXTURE:
        {
            SceneShading s = {};
            s.tex_table = T.tex_table; s.tex_data = T.tex_data;
            sample_texture(s, index_in(v[0], T.n_tex), v[1], v[2], r);
            const CutoutView cv { T.cutout_tab, T.uvs, T.tex_table, T.tex_data };
            r[4] = cutout_accept(cv, (size_t)index_in(v[3], T.n_attr), v[4], v[5]) ? 1.0f : 0.0f;
            break;
        }
        case SHADING_BRDF_TERMS:
        {
            const float roughness = v[18], ndoth = v[19], ndotl = v[20], ndotv = v[21], vdoth = v[22];
            r[0] = D_ggx(ndoth, roughness * roughness);
            r[1] = G_schlick_ggx(ndotl, ndotv, roughness);
            const f3 F = F_schlick(in3(v, 12), vdoth);
            out3(r, 2, F);
            out3(r, 5, evaluate_specular_brdf(roughness, F, ndoth, ndotl, ndotv));
            break;
        }
        case SHADING_BRDF_UBER:
            out3(r, 0, evaluate_uber_brdf(in3(v, 15), v[18], in3(v, 0), in3(v, 12), in3(v, 3), in3(v, 9), in3(v, 6)));
            out3(r, 3, fresnel_schlick_roughness(v[21], in3(v, 12), v[18]));
            break;
        case SHADING_LOBES:
            out3(r, 0, sample_cosine_lobe_n(in3(v, 0), v[3], v[4]));
            out3(r, 3, sample_cosine_lobe(in3(v, 0), v[3], v[4]));
            out3(r, 6, importance_sample_ggx(v[3], v[4], in3(v, 0), v[5]));
            out3(r, 9, sample_specular_ggx_lobe(in3(v, 0), v[5], v[3], v[4]));
            break;
        case SHADING_LIGHT_HARD:
        case SHADING_LIGHT_SHADOW:
        {
            hr_light L = T.light;   // the colour; the rest of the light is the element's
            for (int k = 0; k < 4; k++) { L.data0[k] = v[11 + k]; L.data1[k] = v[15 + k]; }
            L.data3[0] = v[19]; L.data3[1] = v[20]; L.data3[2] = v[21];
            if (mode == SHADING_LIGHT_HARD)
            {
                f3 Li, Wi, Wh;
                fetch_light_hard(L, in3(v, 6), in3(v, 0), in3(v, 3), Li, Wi, Wh, r[9], r[10]);
                out3(r, 0, Li); out3(r, 3, Wi); out3(r, 6, Wh);
            }
            else
            {
                f3 Wi;
                fetch_light_shadow(L, in3(v, 0), in3(v, 3), v[9], v[10], Wi, r[3], r[4]);
                out3(r, 0, Wi);
            }
            break;
        }
        case SHADING_GI_OCT:
            gi_oct_encode(in3(v, 0), r[0], r[1]);
            out3(r, 2, gi_oct_decode(v[3], v[4]));
            out3(r, 5, probe_location(T.d, index_in(v[5], T.d.probe_counts[0] * T.d.probe_counts[1] * T.d.probe_counts[2])));
            out3(r, 8, spherical_fibonacci(v[6], v[7]));
            break;
        case SHADING_GI_COORDS:
        {
            const int tw = (int)v[4], th = (int)v[5], side = (int)v[6], col = (int)v[7], row = (int)v[8];
            const int per_row = side >= 0 ? (tw - 2) / (side + 2) : 0;
            if (per_row <= 0) break;
            texture_coord_from_direction(in3(v, 0), row * per_row + col, tw, th, side, r[0], r[1]);
            const DivBy Dw = div_prepare((float)tw), Dh = div_prepare((float)th);
            texture_coord_from_cell(in3(v, 0), col, row, Dw, Dh, false, side, r[2], r[3]);
            const bool in = atlas_div_inrange(Dw, Dh);   // forced on only inside div_by_inrange's domain
            texture_coord_from_cell(in3(v, 0), col, row, Dw, Dh, in, side, r[4], r[5]);
            r[6] = in ? 1.0f : 0.0f;
            break;
        }
        case SHADING_GATHER:
        {
            const AtlasRGBA irr { T.irradiance, T.d.irradiance_texture_width, T.d.irradiance_texture_height };
            const AtlasRG   dep { T.depth, T.d.depth_texture_width, T.d.depth_texture_height };
            out3(r, 0, atlas_bilinear_rgb(irr, v[0], v[1]));
            atlas_bilinear_rg(dep, v[0], v[1], r[3], r[4]);
            out3(r, 5, sample_irradiance_net(T.d, in3(v, 2), in3(v, 5), in3(v, 8), irr, dep));
            out3(r, 8, sample_irradiance(T.d, in3(v, 2), in3(v, 5), in3(v, 8), irr, dep));
            break;
        }
        case SHADING_SURFACE:
        {
            const int flags = (int)v[3];
            SceneShading s = {};
            s.positions = T.positions; s.tri_material = T.tri_material; s.materials = T.materials;
            s.normals   = (flags & 1) ? T.normals : nullptr;
            if (flags & 4) { s.uvs = T.tri_uvs; s.mat_tex = T.mat_tex; s.tex_table = T.tex_table; s.tex_data = T.tex_data; }
            s.tangents  = (flags & 8) ? T.tangents : nullptr;
            const SurfaceHit o = surface_from(s, (size_t)index_in(v[0], T.n_tris), (flags & 2) ? T.inst_m : nullptr, v[1], v[2]);
            out3(r, 0, o.P); out3(r, 3, o.N); out3(r, 6, o.albedo); r[9] = o.roughness; r[10] = o.metallic;
            break;
        }
        default: break;
    }
}

__global__ __launch_bounds__(256) void k_selftest_shading(int mode, long long n, const float* __restrict__ in, ShadingTables T, int nout, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[SHADING_IN], r[SHADING_MAX_OUT];
    for (int k = 0; k < SHADING_IN; k++) v[k] = in[i * SHADING_IN + k];
    for (int k = 0; k < SHADING_MAX_OUT; k++) r[k] = 0.0f;
    shading_eval(mode, v, T, r);
    for (int k = 0; k < nout; k++) out[(size_t)k * n + i] = r[k];
}

} // namespace

extern "C" hr_status hr_selftest_shading(int32_t mode, int64_t n, const float* in, const void* tables, int32_t nout, float* out, void* stream)
{
    HR_CHECK_ARG(mode >= 0 && mode < SHADING_MODE_COUNT && n >= 0 && n <= SHADING_MAX_N && tables && nout >= 1 && nout <= SHADING_MAX_OUT);
    HR_CHECK_ARG(n == 0 || (in && out));
    ShadingTables T;
    std::memcpy(&T, tables, sizeof(T));
    // every table a mode reads is there and has the extents its clamps assume
    if (mode == SHADING_CUBE)
        HR_CHECK_ARG(T.cube && T.cube_size > 0 && T.prefiltered && T.pre_levels > 0 && T.pre_levels < 31 && T.pre_size > 0 && (T.pre_size >> (T.pre_levels - 1)) > 0 && T.lut && T.lut_size > 0);
    if (mode == SHADING_TEXTURE) HR_CHECK_ARG(T.tex_table && T.tex_data && T.cutout_tab && T.uvs && T.n_tex > 0 && T.n_attr > 0);
    if (mode == SHADING_GI_OCT || mode == SHADING_GATHER) HR_CHECK_ARG(T.d.probe_counts[0] > 0 && T.d.probe_counts[1] > 0 && T.d.probe_counts[2] > 0 && T.d.probe_counts[0] <= 1024 && T.d.probe_counts[1] <= 1024 && T.d.probe_counts[2] <= 1024);
    if (mode == SHADING_GATHER)
    {
        const hr_ddgi_uniforms& d = T.d;
        HR_CHECK_ARG(T.irradiance && T.depth && d.irradiance_probe_side_length > 0 && d.depth_probe_side_length > 0);
        // the atlas is probe_counts.x * probe_counts.y cells wide and probe_counts.z high (hr_ddgi_create): what the gather's cell addressing assumes
        HR_CHECK_ARG(d.irradiance_texture_width == (d.irradiance_probe_side_length + 2) * d.probe_counts[0] * d.probe_counts[1] + 2 && d.irradiance_texture_height == (d.irradiance_probe_side_length + 2) * d.probe_counts[2] + 2);
        HR_CHECK_ARG(d.depth_texture_width == (d.depth_probe_side_length + 2) * d.probe_counts[0] * d.probe_counts[1] + 2 && d.depth_texture_height == (d.depth_probe_side_length + 2) * d.probe_counts[2] + 2);
    }
    // SURFACE trusts the tables' material and texture indices (the tests build them; hr_scene_create validates a scene's)
    if (mode == SHADING_SURFACE) HR_CHECK_ARG(T.positions && T.normals && T.tangents && T.tri_uvs && T.tri_material && T.materials && T.mat_tex && T.inst_m && T.tex_table && T.tex_data && T.n_tris > 0 && T.n_mats > 0);
    if (n == 0) return HR_OK;
    hipLaunchKernelGGL(k_selftest_shading, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)mode, (long long)n, in, T, (int)nout, out);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
