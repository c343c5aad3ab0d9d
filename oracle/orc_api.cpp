// ORACLE — TEST INFRASTRUCTURE ONLY (see orc_api.h).
#include "orc_api.h"
#include "orc_bvh.h"
#include "orc_common.h"
#include "orc_reproject.h"
#include <atomic>

using namespace orc;

extern "C" {

void* orc_scene_create(const float* verts, int n_tris, const float* normals, const uint32_t* tri_material, const uint32_t* tri_mesh_id, const float* materials, int n_materials)
{
    Scene* s = new Scene();
    s->build(verts, n_tris);
    if (normals) s->tri_normals.assign(normals, normals + (size_t)n_tris * 9);
    if (tri_material) s->tri_material.assign(tri_material, tri_material + n_tris);
    if (tri_mesh_id) s->tri_mesh_id.assign(tri_mesh_id, tri_mesh_id + n_tris);
    if (materials) s->materials.assign(materials, materials + (size_t)n_materials * 8);
    return s;
}
// textured materials: uvs [n][3][2], tangents [n][3][3] (nullable), mat_tex [m][6], textures: n_tex RGBA8 images
void orc_scene_set_textures(void* scene, const float* uvs, const float* tangents, const int32_t* mat_tex, int n_materials, int n_tex,
                            const uint8_t* const* tex_rgba, const int32_t* tex_w, const int32_t* tex_h)
{
    Scene*       s = (Scene*)scene;
    const size_t n = s->tris.size();
    if (uvs) s->tri_uvs.assign(uvs, uvs + n * 6);
    if (tangents) s->tri_tangents.assign(tangents, tangents + n * 9);
    s->mat_tex.assign(mat_tex, mat_tex + (size_t)n_materials * 6);
    s->textures.resize(n_tex);
    for (int i = 0; i < n_tex; i++)
    {
        s->textures[i].w = tex_w[i]; s->textures[i].h = tex_h[i];
        s->textures[i].rgba.assign(tex_rgba[i], tex_rgba[i] + (size_t)tex_w[i] * tex_h[i] * 4);
    }
}
void orc_instances_flatten(int n_instances, const float* matrices, const uint32_t* first_tri, const uint32_t* mesh_tri_base, const uint32_t* n_tris,
                           const float* mesh_positions, const float* mesh_normals, float* out_positions, float* out_normals)
{
    for (int i = 0; i < n_instances; i++)
    {
        const float* m = matrices + (size_t)i * 16;
        for (uint32_t t = 0; t < n_tris[i]; t++)
            for (int v = 0; v < 3; v++)
            {
                const float* p = mesh_positions + ((size_t)mesh_tri_base[i] + t) * 9 + v * 3;
                float*       o = out_positions + ((size_t)first_tri[i] + t) * 9 + v * 3;
                for (int r = 0; r < 3; r++) o[r] = ((m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2]) + m[12 + r] * 1.0f;
                if (mesh_normals && out_normals)
                {
                    const float* n = mesh_normals + ((size_t)mesh_tri_base[i] + t) * 9 + v * 3;
                    float*       q = out_normals + ((size_t)first_tri[i] + t) * 9 + v * 3;
                    for (int r = 0; r < 3; r++) q[r] = (m[r] * n[0] + m[4 + r] * n[1]) + m[8 + r] * n[2];
                }
            }
    }
}
void orc_scene_set_instances(void* scene, int n_instances, const float* matrices, const uint32_t* first_tri, const uint32_t* mesh_tri_base, const uint32_t* mesh_id,
                             const uint32_t* n_tris, int n_mesh_tris, const float* mesh_positions, const float* mesh_normals, const uint32_t* mesh_material,
                             const float* mesh_uvs, const float* mesh_tangents)
{
    Scene* s = (Scene*)scene;
    s->instances.resize((size_t)n_instances);
    s->tri_instance.assign(s->tris.size(), 0u);
    for (int i = 0; i < n_instances; i++)
    {
        Scene::Instance& r = s->instances[(size_t)i];
        for (int k = 0; k < 16; k++) r.m[k] = matrices[(size_t)i * 16 + k];
        r.first_tri = first_tri[i]; r.mesh_tri_base = mesh_tri_base[i]; r.mesh_id = mesh_id[i]; r.n_tris = n_tris[i];
        for (uint32_t t = 0; t < r.n_tris; t++) s->tri_instance[(size_t)r.first_tri + t] = (uint32_t)i;
    }
    const size_t n = (size_t)n_mesh_tris;
    s->mesh_positions.assign(mesh_positions, mesh_positions + n * 9);
    if (mesh_normals) s->mesh_normals.assign(mesh_normals, mesh_normals + n * 9);
    if (mesh_material) s->mesh_material.assign(mesh_material, mesh_material + n);
    if (mesh_uvs) s->mesh_uvs.assign(mesh_uvs, mesh_uvs + n * 6);
    if (mesh_tangents) s->mesh_tangents.assign(mesh_tangents, mesh_tangents + n * 9);
}
void orc_scene_destroy(void* scene) { delete (Scene*)scene; }
int  orc_scene_num_nodes(const void* scene) { return (int)((const Scene*)scene)->nodes.size(); }
// on != 0: every query of this scene, those of the passes' hit shaders included, tests every triangle (tests/closest_cases.py)
void orc_scene_set_brute_force(void* scene, int on) { ((Scene*)scene)->brute_force = on != 0; }

// single-ray entry points: the ray-query / traceRay mock of oracle/refshim calls these through a function pointer
int orc_any_hit_one(void* scene, const float* o, const float* d, float t_min, float t_max)
{
    return ((const Scene*)scene)->any_hit(v3(o[0], o[1], o[2]), v3(d[0], d[1], d[2]), t_min, t_max) ? 1 : 0;
}
int orc_closest_hit_one(void* scene, const float* o, const float* d, float t_min, float t_max, float* tuv)
{
    Hit h = ((const Scene*)scene)->closest_hit(v3(o[0], o[1], o[2]), v3(d[0], d[1], d[2]), t_min, t_max);
    tuv[0] = h.t; tuv[1] = h.u; tuv[2] = h.v;
    return h.prim;
}

void orc_any_hit_batch(const void* scene, int n, const float* rays, uint8_t* out, int brute_force, uint64_t* stats)
{
    const Scene& s = *(const Scene*)scene;
    if (stats)
    {
        traversal_stats() = TraversalStats();
        // serial, instrumented
        for (int i = 0; i < n; i++)
        {
            const float* r = rays + (size_t)i * 8;
            out[i] = s.any_hit(v3(r[0], r[1], r[2]), v3(r[4], r[5], r[6]), r[7], r[3]) ? 1 : 0;
        }
        stats[0] = traversal_stats().nodes;
        stats[1] = traversal_stats().tris;
        return;
    }
#pragma omp parallel for schedule(dynamic, 256)
    for (int i = 0; i < n; i++)
    {
        const float* r = rays + (size_t)i * 8;
        vec3 o = v3(r[0], r[1], r[2]), d = v3(r[4], r[5], r[6]);
        bool h = brute_force ? s.any_hit_brute(o, d, r[7], r[3]) : s.any_hit(o, d, r[7], r[3]);
        out[i] = h ? 1 : 0;
    }
}

void orc_closest_hit_batch(const void* scene, int n, const float* rays, float* out_tuv, int32_t* out_prim, int brute_force)
{
    const Scene& s = *(const Scene*)scene;
#pragma omp parallel for schedule(dynamic, 256)
    for (int i = 0; i < n; i++)
    {
        const float* r = rays + (size_t)i * 8;
        vec3 o = v3(r[0], r[1], r[2]), d = v3(r[4], r[5], r[6]);
        Hit  h = brute_force ? s.closest_hit_brute(o, d, r[7], r[3]) : s.closest_hit(o, d, r[7], r[3]);
        out_tuv[(size_t)i * 3 + 0] = h.t;
        out_tuv[(size_t)i * 3 + 1] = h.u;
        out_tuv[(size_t)i * 3 + 2] = h.v;
        out_prim[i]                = h.prim;
    }
}

// ---------------------------------------------------------------------------------------
// G-buffer synthesis by primary-ray casting.  Output conventions follow g_buffer.frag:86-112:
//   GB1 RGBA8  = albedo.rgb, metallic
//   GB2 RGBA16F = octahedral normal.xy, motion (prev_uv - cur_uv)          (:47-67,103)
//   GB3 RGBA16F = roughness, curvature, mesh id, linear z (= clip z)         (:106-111)
//   depth F32  = clip.z / clip.w, sky = 1.0;  GB3 sky = (0,0,0,-1)           (g_buffer.cpp:88,96)
// Test tooling, not a restatement of a reference shader (the reference rasterises).
static inline vec3 tri_normal_at(const Scene& s, int prim, float b0, float b1, float b2)
{
    if (!s.tri_normals.empty())
    {
        const float* n = &s.tri_normals[(size_t)prim * 9];
        return v3(n[0] * b0 + n[3] * b1 + n[6] * b2, n[1] * b0 + n[4] * b1 + n[7] * b2, n[2] * b0 + n[5] * b1 + n[8] * b2);
    }
    const Tri& t = s.tris[prim];
    return normalize(cross(t.v1 - t.v0, t.v2 - t.v0));
}

static inline bool plane_bary(const Tri& t, vec3 o, vec3 d, float* b0, float* b1, float* b2)
{
    vec3  e1 = t.v1 - t.v0, e2 = t.v2 - t.v0;
    vec3  n  = cross(e1, e2);
    float dn = dot(n, d);
    if (dn == 0.0f) return false;
    float tt = dot(n, t.v0 - o) / dn;
    vec3  p  = (o + d * tt) - t.v0;
    float d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), p1 = dot(p, e1), p2 = dot(p, e2);
    float den = d11 * d22 - d12 * d12;
    if (den == 0.0f) return false;
    *b1 = (d22 * p1 - d12 * p2) / den;
    *b2 = (d11 * p2 - d12 * p1) / den;
    *b0 = 1.0f - *b1 - *b2;
    return true;
}

void orc_gbuffer_raycast(const void* scene_, const void* ubo_, int w, int h, uint8_t* gb1, uint16_t* gb2, uint16_t* gb3, float* depth)
{
    const Scene& s   = *(const Scene*)scene_;
    const UBO&   ubo = *(const UBO*)ubo_;
    const vec3   cam = v3(ubo.cam_pos[0], ubo.cam_pos[1], ubo.cam_pos[2]);
    auto pixel_dir = [&](float px, float py) {
        float u = px / (float)w, v = py / (float)h;
        vec3  far_p = world_position_from_depth(u, v, 1.0f, ubo.view_proj_inverse);
        return normalize(far_p - cam);
    };
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
        {
            size_t   i  = (size_t)y * w + x;
            uint8_t* o1 = gb1 + i * 4;
            uint16_t *o2 = gb2 + i * 4, *o3 = gb3 + i * 4;
            vec3 d  = pixel_dir((float)x + 0.5f, (float)y + 0.5f);
            Hit  hit = s.closest_hit(cam, d, 0.0f, 1.0e30f);
            if (hit.prim < 0)
            {
                o1[0] = o1[1] = o1[2] = o1[3] = 0;
                o2[0] = o2[1] = o2[2] = o2[3] = 0;
                o3[0] = o3[1] = o3[2] = 0;
                o3[3] = f32_to_f16(-1.0f);
                depth[i] = 1.0f;
                continue;
            }
            vec3  P    = cam + d * hit.t;
            vec4  clip = mul(ubo.view_proj, vec4 { P.x, P.y, P.z, 1.0f });
            vec4  pclip = mul(ubo.prev_view_proj, vec4 { P.x, P.y, P.z, 1.0f });
            float b0 = 1.0f - hit.u - hit.v;
            vec3  nI = tri_normal_at(s, hit.prim, b0, hit.u, hit.v); // un-normalised interpolated normal
            vec3  n  = normalize(nI);
            if (dot(n, d) > 0.0f) n = -n; // face the viewer (two-sided)
            // curvature = sqrt(max(|dFdx N|^2, |dFdy N|^2)) with attribute extrapolation over the triangle plane
            float curvature = 0.0f;
            {
                float c0, c1, c2;
                vec3  dxv = v3(0, 0, 0), dyv = v3(0, 0, 0);
                if (plane_bary(s.tris[hit.prim], cam, pixel_dir((float)x + 1.5f, (float)y + 0.5f), &c0, &c1, &c2)) dxv = tri_normal_at(s, hit.prim, c0, c1, c2) - nI;
                if (plane_bary(s.tris[hit.prim], cam, pixel_dir((float)x + 0.5f, (float)y + 1.5f), &c0, &c1, &c2)) dyv = tri_normal_at(s, hit.prim, c0, c1, c2) - nI;
                if (s.tri_normals.empty()) { dxv = v3(0, 0, 0); dyv = v3(0, 0, 0); }
                curvature = std::sqrt(fmax2(dot(dxv, dxv), dot(dyv, dyv)));
            }
            vec2  oct = direction_to_octohedral(n);
            float cx = clip.x / clip.w * 0.5f + 0.5f, cy = clip.y / clip.w * 0.5f + 0.5f;
            float px = pclip.x / pclip.w * 0.5f + 0.5f, py = pclip.y / pclip.w * 0.5f + 0.5f;
            uint32_t mat = s.tri_material.empty() ? 0u : s.tri_material[hit.prim];
            float albedo[3] = { 0.8f, 0.8f, 0.8f }, metallic = 0.0f, roughness = 0.5f;
            if (!s.materials.empty())
            {
                const float* m = &s.materials[(size_t)mat * 8];
                albedo[0] = m[0]; albedo[1] = m[1]; albedo[2] = m[2]; metallic = m[3]; roughness = m[4];
            }
            for (int c = 0; c < 3; c++) o1[c] = (uint8_t)(clampf(albedo[c], 0.0f, 1.0f) * 255.0f + 0.5f);
            o1[3] = (uint8_t)(clampf(metallic, 0.0f, 1.0f) * 255.0f + 0.5f);
            o2[0] = f32_to_f16(oct.x); o2[1] = f32_to_f16(oct.y);
            o2[2] = f32_to_f16(px - cx); o2[3] = f32_to_f16(py - cy);
            float mesh_id = s.tri_mesh_id.empty() ? 0.0f : (float)s.tri_mesh_id[hit.prim];
            o3[0] = f32_to_f16(fmax2(roughness, 0.1f)); o3[1] = f32_to_f16(curvature);
            o3[2] = f32_to_f16(mesh_id); o3[3] = f32_to_f16(clip.z);
            float dd = clip.z / clip.w;
            depth[i] = dd >= 1.0f ? 0.99999994f : dd;
        }
}

// ---- scalar helpers ---------------------------------------------------------------------
uint16_t orc_f32_to_f16(float f) { return f32_to_f16(f); }
float    orc_f16_to_f32(uint16_t h) { return f16_to_f32(h); }
void     orc_sincos(float x, float* s, float* c) { det_sincos(x, s, c); }
float    orc_exp(float x) { return det_exp(x); }
float    orc_log(float x) { return det_log(x); }
float    orc_pow(float x, float y) { return det_pow_auto(x, y); }
void     orc_oct_decode(float ex, float ey, float* out3)
{
    vec3 v = octohedral_to_direction(ex, ey);
    out3[0] = v.x; out3[1] = v.y; out3[2] = v.z;
}
void orc_oct_encode(const float* n3, float* out2)
{
    vec2 v = direction_to_octohedral(v3(n3[0], n3[1], n3[2]));
    out2[0] = v.x; out2[1] = v.y;
}
float orc_sample_blue_noise(int x, int y, int sample_index, int dim, const uint8_t* sobol, const uint8_t* scrambling_ranking)
{
    BlueNoise bn { sobol, scrambling_ranking };
    return sample_blue_noise(x, y, sample_index, dim, bn);
}
void orc_world_position_from_depth(float u, float v, float depth, const float* view_proj_inverse, float* out3)
{
    mat4 m;
    for (int i = 0; i < 16; i++) m.m[i] = view_proj_inverse[i];
    vec3 p = world_position_from_depth(u, v, depth, m);
    out3[0] = p.x; out3[1] = p.y; out3[2] = p.z;
}
}

// ---- self-test mirror (hr_selftest_math_sweep / hr_selftest_fast_math, include/hr_api_post.h) ----------------------
// The same modes, the same index-generated inputs and the same planar outputs as the device self test, on arrays and in
// parallel, so that sweeps over all 2^32 fp32 patterns can be checked chunk by chunk without moving inputs through Python.
namespace {

struct SelftestParams
{
    float    m[16], m2[16], cam[3], y, z, w, h, cur_id;
    uint32_t d_first;
    int32_t  n_num;
    float    num[32];
    float    pad[6];
};
static_assert(sizeof(SelftestParams) == 80 * 4, "SelftestParams layout");
constexpr int MAX_OUT = 9;

float random_numerator(uint64_t j)
{
    uint64_t z = j * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 29)) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 32;
    const uint32_t lo = 0x2b8cbcccu, hi = 0x48927c00u;   // bits of 1e-12f and 3e5f
    const uint32_t b  = lo + (uint32_t)((z & 0xffffffffull) % (uint64_t)(hi - lo + 1u));
    return u2f(b | ((uint32_t)(z >> 63) << 31));
}

void inputs(int gen, int64_t i, int64_t first, const float* in, const SelftestParams& P, float v[8])
{
    for (int k = 0; k < 8; k++) v[k] = 0.0f;
    const uint64_t j = (uint64_t)(first + i);
    if (gen == 0)
    {
        for (int k = 0; k < 8; k++) v[k] = in[i * 8 + k];
        return;
    }
    v[1] = P.y;
    v[2] = P.z;
    if (gen == 1) v[0] = u2f((uint32_t)j);
    else if (gen == 2)
    {
        v[0] = f16_to_f32((uint16_t)(j & 0xffffu));
        v[1] = f16_to_f32((uint16_t)((j >> 16) & 0xffffu));
    }
    else if (gen == 3)
    {
        const uint64_t nn = (uint64_t)(P.n_num > 0 ? P.n_num : 1);
        const float    t  = P.num[j % nn];
        v[0] = t != t ? random_numerator(j) : t;
        v[1] = u2f(P.d_first + (uint32_t)(j / nn));
    }
}

mat4 to_mat4(const float* m)
{
    mat4 r;
    for (int k = 0; k < 16; k++) r.m[k] = m[k];
    return r;
}

// tu 0: device_math.h (api.hip), every mode has a definition here.  tu 1: denoise_fast_resolve.hip; modes 0-2 and 4 are the hardware's
// approximations (rcp, rsq, exp, log, oct_unit): their accuracy is measured against float64 by the tests, they have no oracle here.
bool eval(int tu, int which, const float v[8], const SelftestParams& P, float r[MAX_OUT])
{
    const float x = v[0], y = v[1], z = v[2];
    for (int k = 0; k < MAX_OUT; k++) r[k] = 0.0f;
    if (tu == 0)
    {
        switch (which)
        {
            case 0: det_sincos(x, &r[0], &r[1]); return true;
            case 1: r[0] = det_exp(x); return true;
            case 2: r[0] = det_log(x); return true;
            case 3: r[0] = det_pow_auto(x, y); return true;
            case 4: r[0] = (float)f32_to_f16(x); r[1] = f16_to_f32(f32_to_f16(x)); return true;
            case 5: { vec3 o = octohedral_to_direction(x, y); r[0] = o.x; r[1] = o.y; r[2] = o.z; return true; }
            case 6: { vec2 o = direction_to_octohedral(v3(x, y, z)); r[0] = o.x; r[1] = o.y; return true; }
            case 7: r[0] = std::sqrt(x); r[1] = 1.0f / x; return true;
            case 8: r[0] = x / y; return true;
            case 9: r[0] = r[1] = r[2] = x / y; return true;   // div_by, div_by_inrange, div_by_if: correctly rounded (inrange: in its domain)
            case 10: r[0] = glsl_min(x, y); r[1] = glsl_max(x, y); r[2] = glsl_clamp(x, y, z); return true;
            case 11: r[0] = fmin2(x, y); r[1] = fmax2(x, y); r[2] = clampf(x, y, z); return true;
            case 12: r[0] = mixf(x, y, z); r[1] = smoothstepf(x, y, z); r[2] = stepf(x, y); r[3] = fractf(x); return true;
            case 13: r[0] = det_powi(x, (y >= 0.0f && y <= 64.0f) ? (int)y : 0); r[1] = det_pow(x, y); return true;
            case 14: { vec3 o = world_position_from_depth(x, y, z, to_mat4(P.m)); r[0] = o.x; r[1] = o.y; r[2] = o.z; return true; }
            default: return false;
        }
    }
    const int w = (int)P.w, h = (int)P.h;
    switch (which)
    {
        case 3: r[0] = (float)f32_to_f16(x); r[1] = (float)f32_to_f16(y); return true;
        case 5: r[0] = mixf(x, y, z); r[1] = x - y * y; r[2] = x * y + z; r[3] = x * y; r[4] = std::fabs(x * x - y); return true;
        case 6: r[0] = mixf(mixf(v[0], v[1], v[4]), mixf(v[2], v[3], v[4]), v[5]); return true;
        case 7:
        {
            // gi_common.glsl texture_coord_from_direction, then the bilinear set-up's texel coordinate u * size - 0.5
            const float tw = v[5], th = v[6], side = (float)(int)v[4], pwb = side + 2.0f;
            const float zx = (x + 1.0f) * 0.5f, zy = (y + 1.0f) * 0.5f;
            const float u = ((float)(int)v[2] * pwb + 2.0f) / tw + (zx * side) / tw, vv = ((float)(int)v[3] * pwb + 2.0f) / th + (zy * side) / th;
            r[0] = u * tw - 0.5f;
            r[1] = vv * th - 0.5f;
            return true;
        }
        case 8: r[0] = x / y; r[1] = (float)(int)std::floor((x + y * z) * v[3]); return true;
        case 9:
        {
            const int   px = (int)x, py = (int)y;
            const mat4  M  = to_mat4(P.m);
            const float tu = ((float)px + 0.5f) / (float)w, tv = ((float)py + 0.5f) / (float)h;
            const uint32_t c2x = f2u(v[3]), c2y = f2u(v[4]), q2x = f2u(v[5]), q3y = f2u(v[6]);
            const vec3  cn = octohedral_to_direction(f16_to_f32(c2x & 0xffffu), f16_to_f32(c2x >> 16));
            const vec3  cp = world_position_from_depth(tu, tv, z, M);
            const vec3  hn = octohedral_to_direction(f16_to_f32(q2x & 0xffffu), f16_to_f32(q2x >> 16));
            const vec3  hp = world_position_from_depth(tu + f16_to_f32(c2y & 0xffffu), tv + f16_to_f32(c2y >> 16), v[7], M);
            r[0] = is_reprojection_valid(px, py, cp, hp, cn, hn, P.cur_id, f16_to_f32(q3y & 0xffffu), w, h) ? 1.0f : 0.0f;
            return true;
        }
        case 10:
        {
            const vec2 o = virtual_point_reprojection((int)x, (int)y, w, h, z, v[3], v3(P.cam[0], P.cam[1], P.cam[2]), to_mat4(P.m), to_mat4(P.m2));
            r[0] = o.x; r[1] = o.y;
            return true;
        }
        case 11:
        {
            const float tu = ((float)(int)x + 0.5f) / (float)w, tv = ((float)(int)y + 0.5f) / (float)h;
            const vec3  Pw = world_position_from_depth(tu, tv, z, to_mat4(P.m));
            const uint32_t g2x = f2u(v[3]);
            const vec3  N  = octohedral_to_direction(f16_to_f32(g2x & 0xffffu), f16_to_f32(g2x >> 16));
            const vec3  Wo = normalize(v3(P.cam[0], P.cam[1], P.cam[2]) - Pw);
            r[0] = Pw.x; r[1] = Pw.y; r[2] = Pw.z; r[3] = N.x; r[4] = N.y; r[5] = N.z; r[6] = Wo.x; r[7] = Wo.y; r[8] = Wo.z;
            return true;
        }
        default: return false;
    }
}

// planes that hold fp16 bit patterns (as floats): any two fp16 NaNs are equal there
bool half_plane(int tu, int which, int k) { return (tu == 0 && which == 4 && k == 0) || (tu == 1 && which == 3); }

bool same(float a, float b, bool half)
{
    if (f2u(a) == f2u(b) || (a != a && b != b)) return true;
    if (!half || !(a >= 0.0f && a < 65536.0f && b >= 0.0f && b < 65536.0f)) return false;
    const uint32_t ha = (uint32_t)a, hb = (uint32_t)b;
    return a == (float)ha && b == (float)hb && (ha & 0x7c00u) == 0x7c00u && (hb & 0x7c00u) == 0x7c00u && (ha & 0x3ffu) && (hb & 0x3ffu);
}

} // namespace

extern "C" {

// out: [nout][n] floats.  Returns 0, or -1 for a mode without a definition here / bad arguments.
int orc_selftest_math(int tu, int which, int gen, int64_t first, int64_t n, const float* in, const float* params, int nout, float* out)
{
    if (nout < 1 || nout > MAX_OUT || n < 0 || (gen == 0 && !in) || gen < 0 || gen > 3) return -1;
    SelftestParams P;
    std::memcpy(&P, params, sizeof(P));
    {
        float v[8], r[MAX_OUT];
        inputs(1, 0, 0, nullptr, P, v);
        if (!eval(tu, which, v, P, r)) return -1;
    }
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++)
    {
        float v[8], r[MAX_OUT];
        inputs(gen, i, first, in, P, v);
        eval(tu, which, v, P, r);
        for (int k = 0; k < nout; k++) out[(size_t)k * n + i] = r[k];
    }
    return 0;
}

// Compares the device's planar outputs of one chunk with the mirror, NaN == NaN (tests/helpers.assert_bits_equal_nan).  Returns the number of
// mismatching elements (or -1); the first max_report of them (in no particular order) go to report_out as chunk-relative indices.
int64_t orc_selftest_compare(int tu, int which, int gen, int64_t first, int64_t n, const float* in, const float* params, int nout, const float* gpu_out,
                             int64_t max_report, int64_t* report_out)
{
    if (nout < 1 || nout > MAX_OUT || n < 0 || (gen == 0 && !in) || gen < 0 || gen > 3) return -1;
    SelftestParams P;
    std::memcpy(&P, params, sizeof(P));
    {
        float v[8], r[MAX_OUT];
        inputs(1, 0, 0, nullptr, P, v);
        if (!eval(tu, which, v, P, r)) return -1;
    }
    int64_t              bad = 0;
    std::atomic<int64_t> slot { 0 };
#pragma omp parallel for schedule(static) reduction(+ : bad)
    for (int64_t i = 0; i < n; i++)
    {
        float v[8], r[MAX_OUT];
        inputs(gen, i, first, in, P, v);
        eval(tu, which, v, P, r);
        bool ok = true;
        for (int k = 0; k < nout; k++) ok = ok && same(r[k], gpu_out[(size_t)k * n + i], half_plane(tu, which, k));
        if (!ok)
        {
            bad++;
            const int64_t s = slot.fetch_add(1);
            if (s < max_report) report_out[s] = i;
        }
    }
    return bad;
}
}
