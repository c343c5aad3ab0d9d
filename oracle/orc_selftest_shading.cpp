// ORACLE — TEST INFRASTRUCTURE ONLY (see orc_math.h header).
// Mirror of the device's hr_selftest_shading (hybrid_rendering_amd/csrc/selftest_shading.h: modes, element layout, table block): the oracle's own
// shading functions (orc_shading.h, orc_ao.cpp, orc_shadows.cpp) on arrays, so that tests/test_gpu_shading_layer.py can compare the device with them
// bit for bit and tests/test_shading_cases.py can compare them with a float64 restatement.  Nothing is restated here: every mode calls the function
// the pass restatements call.
#include <cstring>
#include "orc_api.h"
#include "orc_shading.h"

using namespace orc;

namespace {

enum { M_RNG = 0, M_CUBE, M_TEXTURE, M_BRDF_TERMS, M_BRDF_UBER, M_LOBES, M_LIGHT_HARD, M_LIGHT_SHADOW, M_GI_OCT, M_GI_COORDS, M_GATHER, M_SURFACE,
       M_GATHER_TRACE /* the oracle only: GATHER's inputs + 11 probe k -> what the gather decided for that probe (IrrProbeTrace) */, M_COUNT };
constexpr int     N_IN = 24, MAX_OUT = 12;
constexpr int64_t MAX_N = 1 << 17;

struct ShadingTables   // selftest_shading.h, with host pointers
{
    const uint16_t* cube;
    const uint16_t* prefiltered;
    const uint16_t* lut;
    const uint32_t* tex_table;
    const uint8_t*  tex_data;
    const uint32_t* cutout_tab;
    const float*    uvs;
    const uint16_t* irradiance;
    const uint16_t* depth;
    const float*    positions;
    const float*    normals;
    const float*    tangents;
    const float*    tri_uvs;
    const uint32_t* tri_material;
    const float*    materials;
    const int32_t*  mat_tex;
    const float*    inst_m;
    int32_t         cube_size, pre_size, pre_levels, lut_size, n_tex, n_attr, n_tris, n_mats;
    DDGIUniforms    d;
    Light           light;
};
static_assert(sizeof(ShadingTables) == 17 * 8 + 8 * 4 + 88 + 64, "ShadingTables layout");

vec3 in3(const float* v, int k) { return v3(v[k], v[k + 1], v[k + 2]); }
void out3(float* r, int k, vec3 a) { r[k] = a.x; r[k + 1] = a.y; r[k + 2] = a.z; }
int  index_in(float x, int n) { const int i = f2i_sat(x); return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// what the modes need besides the table block, made once per call
struct Prepared
{
    std::vector<Scene::Texture> textures;
    Scene                       surf[16];   // SURFACE: one scene per flag combination
};

void prepare(int mode, const ShadingTables& T, Prepared& P)
{
    if ((mode == M_TEXTURE || mode == M_SURFACE) && T.tex_table && T.tex_data)
        for (int t = 0; t < T.n_tex; t++)
        {
            Scene::Texture x;
            x.w = (int)T.tex_table[t * 4 + 1]; x.h = (int)T.tex_table[t * 4 + 2];
            const uint8_t* src = T.tex_data + (size_t)T.tex_table[t * 4] * 4;
            x.rgba.assign(src, src + (size_t)x.w * x.h * 4);
            P.textures.push_back(x);
        }
    if (mode != M_SURFACE) return;
    const size_t n = (size_t)T.n_tris;
    for (int flags = 0; flags < 16; flags++)
    {
        Scene& s = P.surf[flags];
        s.materials.assign(T.materials, T.materials + (size_t)T.n_mats * 8);
        const std::vector<float>    pos(T.positions, T.positions + n * 9), nrm(T.normals, T.normals + n * 9), tan(T.tangents, T.tangents + n * 9), uv(T.tri_uvs, T.tri_uvs + n * 6);
        const std::vector<uint32_t> mat(T.tri_material, T.tri_material + n);
        if (flags & 4) { s.mat_tex.assign(T.mat_tex, T.mat_tex + (size_t)T.n_mats * 6); s.textures = P.textures; }
        if (flags & 2)
        {
            // one instance of one mesh that holds every triangle: surface_at reads the object-space mesh arrays and the instance's matrix
            Scene::Instance in;
            std::memcpy(in.m, T.inst_m, sizeof(in.m));
            in.first_tri = 0; in.mesh_tri_base = 0; in.mesh_id = 0; in.n_tris = (uint32_t)n;
            s.instances.push_back(in);
            s.tri_instance.assign(n, 0u);
            s.mesh_positions = pos; s.mesh_material = mat;
            if (flags & 1) s.mesh_normals = nrm;
            if (flags & 4) s.mesh_uvs = uv;
            if (flags & 8) s.mesh_tangents = tan;
        }
        else
        {
            s.tris.resize(n);
            for (size_t q = 0; q < n; q++) { s.tris[q].v0 = in3(&pos[q * 9], 0); s.tris[q].v1 = in3(&pos[q * 9], 3); s.tris[q].v2 = in3(&pos[q * 9], 6); }
            s.tri_material = mat;
            if (flags & 1) s.tri_normals = nrm;
            if (flags & 4) s.tri_uvs = uv;
            if (flags & 8) s.tri_tangents = tan;
        }
    }
}

// the alpha test of a cutout material: the hit is ignored iff the albedo texture's alpha at the hit's interpolated uv (surface_at's
// interpolation) is below the material's cutoff; tab: per attribute index { albedo texture + 1 (0: opaque), cutoff bits }
bool cutout_accept(const ShadingTables& T, const Prepared& P, size_t q, float u, float v)
{
    const uint32_t tex1 = T.cutout_tab[q * 2], cutoff = T.cutout_tab[q * 2 + 1];
    if (tex1 == 0u) return true;
    const float  b0 = 1.0f - u - v;
    const float* qu = T.uvs + q * 6;
    const float  tu = (qu[0] * b0 + qu[2] * u) + qu[4] * v;
    const float  tv = (qu[1] * b0 + qu[3] * u) + qu[5] * v;
    return !(sample_texture(P.textures[tex1 - 1u], tu, tv).w < u2f(cutoff));
}

bool checked(int mode, const ShadingTables& T)
{
    const DDGIUniforms& d = T.d;
    const bool grid = d.probe_counts[0] > 0 && d.probe_counts[1] > 0 && d.probe_counts[2] > 0 && d.probe_counts[0] <= 1024 && d.probe_counts[1] <= 1024 && d.probe_counts[2] <= 1024;
    switch (mode)
    {
        case M_CUBE: return T.cube && T.cube_size > 0 && T.prefiltered && T.pre_levels > 0 && T.pre_levels < 31 && T.pre_size > 0 && (T.pre_size >> (T.pre_levels - 1)) > 0 && T.lut && T.lut_size > 0;
        case M_TEXTURE: return T.tex_table && T.tex_data && T.cutout_tab && T.uvs && T.n_tex > 0 && T.n_attr > 0;
        case M_GI_OCT: return grid;
        case M_GATHER:
        case M_GATHER_TRACE:
            return grid && T.irradiance && T.depth && d.irradiance_probe_side_length > 0 && d.depth_probe_side_length > 0 &&
                   d.irradiance_texture_width == (d.irradiance_probe_side_length + 2) * d.probe_counts[0] * d.probe_counts[1] + 2 &&
                   d.irradiance_texture_height == (d.irradiance_probe_side_length + 2) * d.probe_counts[2] + 2 &&
                   d.depth_texture_width == (d.depth_probe_side_length + 2) * d.probe_counts[0] * d.probe_counts[1] + 2 &&
                   d.depth_texture_height == (d.depth_probe_side_length + 2) * d.probe_counts[2] + 2;
        case M_SURFACE: return T.positions && T.normals && T.tangents && T.tri_uvs && T.tri_material && T.materials && T.mat_tex && T.inst_m && T.tex_table && T.tex_data && T.n_tris > 0 && T.n_mats > 0;
        default: return true;
    }
}

void eval(int mode, const float* v, const ShadingTables& T, const Prepared& P, float* r)
{
    switch (mode)
    {
        case M_RNG:
        {
            RNG g = rng_init(f2u(v[0]), f2u(v[1]), f2u(v[2]));
            for (int k = 0; k < 8; k++) r[k] = next_float(g);
            break;
        }
        case M_CUBE:
        {
            const EnvMaps env { CubeH { T.cube, T.cube_size }, T.prefiltered, T.pre_size, T.pre_levels, T.lut, T.lut_size };
            out3(r, 0, env.sky.fetch(in3(v, 0)));
            out3(r, 3, env.prefiltered_fetch(in3(v, 0), v[3]));
            const vec2 l = env.lut_fetch(v[4], v[5]);
            r[6] = l.x; r[7] = l.y;
            break;
        }
        case M_TEXTURE:
        {
            const vec4 c = sample_texture(P.textures[(size_t)index_in(v[0], T.n_tex)], v[1], v[2]);
            r[0] = c.x; r[1] = c.y; r[2] = c.z; r[3] = c.w;
            r[4] = cutout_accept(T, P, (size_t)index_in(v[3], T.n_attr), v[4], v[5]) ? 1.0f : 0.0f;
            break;
        }
        case M_BRDF_TERMS:
        {
            const float roughness = v[18], ndoth = v[19], ndotl = v[20], ndotv = v[21], vdoth = v[22];
            r[0] = D_ggx(ndoth, roughness * roughness);
            r[1] = G_schlick_ggx(ndotl, ndotv, roughness);
            const vec3 F = F_schlick(in3(v, 12), vdoth);
            out3(r, 2, F);
            out3(r, 5, evaluate_specular_brdf(roughness, F, ndoth, ndotl, ndotv));
            break;
        }
        case M_BRDF_UBER:
            out3(r, 0, evaluate_uber_brdf(in3(v, 15), v[18], in3(v, 0), in3(v, 12), in3(v, 3), in3(v, 9), in3(v, 6)));
            out3(r, 3, fresnel_schlick_roughness(v[21], in3(v, 12), v[18]));
            break;
        case M_LOBES:
            // the device keeps two copies of the cosine lobe (shading.h sample_cosine_lobe_n, the AO trace's sample_cosine_lobe); the oracle has one
            out3(r, 0, sample_cosine_lobe(in3(v, 0), v[3], v[4]));
            out3(r, 3, sample_cosine_lobe(in3(v, 0), v[3], v[4]));
            out3(r, 6, importance_sample_ggx(v[3], v[4], in3(v, 0), v[5]));
            out3(r, 9, sample_specular_ggx_lobe(in3(v, 0), v[5], v[3], v[4]));
            break;
        case M_LIGHT_HARD:
        case M_LIGHT_SHADOW:
        {
            Light L = T.light;
            for (int k = 0; k < 4; k++) { L.data0[k] = v[11 + k]; L.data1[k] = v[15 + k]; }
            L.data3[0] = v[19]; L.data3[1] = v[20]; L.data3[2] = v[21];
            if (mode == M_LIGHT_HARD)
            {
                vec3 Li, Wi, Wh;
                fetch_light_hard(L, in3(v, 6), in3(v, 0), in3(v, 3), &Li, &Wi, &Wh, &r[9], &r[10]);
                out3(r, 0, Li); out3(r, 3, Wi); out3(r, 6, Wh);
            }
            else
            {
                vec3 Wi;
                fetch_light_properties_shadow(L, in3(v, 0), in3(v, 3), v[9], v[10], &Wi, &r[3], &r[4]);
                out3(r, 0, Wi);
            }
            break;
        }
        case M_GI_OCT:
        {
            const vec2 e = gi_oct_encode(in3(v, 0));
            r[0] = e.x; r[1] = e.y;
            out3(r, 2, gi_oct_decode(v[3], v[4]));
            out3(r, 5, probe_location(T.d, index_in(v[5], T.d.probe_counts[0] * T.d.probe_counts[1] * T.d.probe_counts[2])));
            out3(r, 8, spherical_fibonacci(v[6], v[7]));
            break;
        }
        case M_GI_COORDS:
        {
            const int tw = f2i_sat(v[4]), th = f2i_sat(v[5]), side = f2i_sat(v[6]), col = f2i_sat(v[7]), row = f2i_sat(v[8]);
            const int per_row = side >= 0 ? (tw - 2) / (side + 2) : 0;
            if (per_row <= 0) break;
            // one definition here: every quotient correctly rounded, whichever way the device's div_by_if goes
            const vec2 c = texture_coord_from_direction(in3(v, 0), row * per_row + col, tw, th, side);
            r[0] = r[2] = r[4] = c.x; r[1] = r[3] = r[5] = c.y;
            r[6] = ((float)tw >= 1e-6f && (float)tw <= 3e5f && (float)th >= 1e-6f && (float)th <= 3e5f) ? 1.0f : 0.0f;
            break;
        }
        case M_GATHER:
        {
            const DDGIUniforms& d = T.d;
            out3(r, 0, atlas_bilinear<4>(T.irradiance, d.irradiance_texture_width, d.irradiance_texture_height, v[0], v[1]));
            const vec3 rg = atlas_bilinear<2>(T.depth, d.depth_texture_width, d.depth_texture_height, v[0], v[1]);
            r[3] = rg.x; r[4] = rg.y;
            out3(r, 5, sample_irradiance_net(d, in3(v, 2), in3(v, 5), in3(v, 8), T.irradiance, T.depth));
            out3(r, 8, sample_irradiance(d, in3(v, 2), in3(v, 5), in3(v, 8), T.irradiance, T.depth));
            break;
        }
        case M_GATHER_TRACE:
        {
            IrrProbeTrace t[8];
            sample_irradiance_net(T.d, in3(v, 2), in3(v, 5), in3(v, 8), T.irradiance, T.depth, t);
            const IrrProbeTrace& p = t[index_in(v[11], 8)];
            r[0] = (float)p.cx; r[1] = (float)p.cy; r[2] = (float)p.cz; r[3] = p.tri[0]; r[4] = p.tri[1]; r[5] = p.tri[2];
            r[6] = p.dist; r[7] = p.mean; r[8] = p.m2; r[9] = p.variance; r[10] = p.weight_before_crush;
            r[11] = (t[0].net_before_nan[0] != t[0].net_before_nan[0] || t[0].net_before_nan[1] != t[0].net_before_nan[1] || t[0].net_before_nan[2] != t[0].net_before_nan[2]) ? 1.0f : 0.0f;
            break;
        }
        case M_SURFACE:
        {
            const int  flags = f2i_sat(v[3]) & 15;
            const Hit  h { 0.0f, v[1], v[2], index_in(v[0], T.n_tris) };
            const SurfaceHit o = surface_at(P.surf[flags], h);
            out3(r, 0, o.P); out3(r, 3, o.N); out3(r, 6, o.albedo); r[9] = o.roughness; r[10] = o.metallic;
            break;
        }
        default: break;
    }
}

} // namespace

extern "C" {

// out: [nout][n] floats.  Returns 0, or -1 for bad arguments / tables a mode needs that are missing or inconsistent.
int orc_selftest_shading(int mode, int64_t n, const float* in, const void* tables, int nout, float* out)
{
    if (mode < 0 || mode >= M_COUNT || n < 0 || n > MAX_N || !tables || nout < 1 || nout > MAX_OUT || (n > 0 && (!in || !out))) return -1;
    ShadingTables T;
    std::memcpy(&T, tables, sizeof(T));
    if (!checked(mode, T)) return -1;
    Prepared P;
    prepare(mode, T, P);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++)
    {
        float r[MAX_OUT];
        for (int k = 0; k < MAX_OUT; k++) r[k] = 0.0f;
        eval(mode, in + i * N_IN, T, P, r);
        for (int k = 0; k < nout; k++) out[(size_t)k * n + i] = r[k];
    }
    return 0;
}

} // extern "C"
