// hr_selftest_shading (selftest_shading.hip): the modes, the element layout and the table block.  The tests' CPU mirror and its Python wrapper
// restate this layout; in = [n][SHADING_IN] floats, out = planar [nout][n].
//   mode            in (float index)                                                        out
//   RNG             0-2 idx, idy, frame (bit patterns)                                      0-7 eight next_float after rng_init
//   CUBE            0-2 d, 3 lod, 4-5 lut (u, v)                                            0-2 CubeMap::fetch, 3-5 prefiltered_fetch, 6-7 lut_fetch
//   TEXTURE         0 texture, 1-2 uv, 3 attribute index, 4-5 barycentrics                  0-3 sample_texture, 4 cutout_accept
//   BRDF_TERMS      12-14 F0, 18 roughness, 19-22 NdotH NdotL NdotV VdotH                   0 D_ggx, 1 G_schlick_ggx, 2-4 F_schlick, 5-7 evaluate_specular_brdf
//   BRDF_UBER       0-2 N, 3-5 Wo, 6-8 Wi, 9-11 Wh, 12-14 F0, 15-17 diffuse, 18, 21         0-2 evaluate_uber_brdf, 3-5 fresnel_schlick_roughness(NdotV)
//   LOBES           0-2 N, 3-4 the two random numbers, 5 roughness / alpha                  0-2 sample_cosine_lobe_n, 3-5 sample_cosine_lobe, 6-8 importance_sample_ggx,
//                                                                                           9-11 sample_specular_ggx_lobe
//   LIGHT_HARD      0-2 P, 3-5 N, 6-8 Wo, 11-14 data0, 15-18 data1, 19-21 data3.xyz         0-2 Li, 3-5 Wi, 6-8 Wh, 9 t_max, 10 attenuation
//   LIGHT_SHADOW    the same + 9-10 the two random numbers                                  0-2 Wi, 3 t_max, 4 attenuation
//   GI_OCT          0-2 v, 3-4 oct, 5 probe index, 6-7 fibonacci (i, n)                     0-1 gi_oct_encode, 2-4 gi_oct_decode, 5-7 probe_location, 8-10 spherical_fibonacci
//   GI_COORDS       0-2 dir, 4-5 atlas extents, 6 side, 7-8 cell (col, row)                 0-1 texture_coord_from_direction, 2-3 texture_coord_from_cell with inrange
//                                                                                           off, 4-5 with it on where atlas_div_inrange allows, 6 atlas_div_inrange
//   GATHER          0-1 (u, v), 2-4 P, 5-7 N, 8-10 Wo                                       0-2 atlas_bilinear_rgb, 3-4 atlas_bilinear_rg, 5-7 sample_irradiance_net,
//                                                                                           8-10 sample_irradiance
//   SURFACE         0 triangle, 1-2 barycentrics, 3 flags (1 vertex normals, 2 the instance      0-2 P, 3-5 N, 6-8 albedo, 9 roughness, 10 metallic of surface_from
//                   matrix, 4 textured materials, 8 tangents)
#pragma once
#include "../../include/hr_api.h"
#include <stdint.h>

enum
{
    SHADING_RNG = 0, SHADING_CUBE, SHADING_TEXTURE, SHADING_BRDF_TERMS, SHADING_BRDF_UBER, SHADING_LOBES, SHADING_LIGHT_HARD, SHADING_LIGHT_SHADOW,
    SHADING_GI_OCT, SHADING_GI_COORDS, SHADING_GATHER, SHADING_SURFACE, SHADING_MODE_COUNT
};
constexpr int     SHADING_IN = 24, SHADING_MAX_OUT = 12;
constexpr int64_t SHADING_MAX_N = 1 << 17;

// by value in the kernel arguments; the pointers are device memory (host memory in the oracle's mirror)
struct ShadingTables
{
    const uint2*    cube;          // [6][cube_size][cube_size] RGBA16F
    const uint2*    prefiltered;   // pre_levels levels of [6][s][s] RGBA16F, s = pre_size >> level
    const uint32_t* lut;           // [lut_size][lut_size] RG16F
    const uint4*    tex_table;     // per texture: texel offset, width, height, 0
    const uint32_t* tex_data;      // RGBA8 texels
    const uint2*    cutout_tab;    // per attribute index: albedo texture + 1 (0: opaque), cutoff bits (cutout.h)
    const float*    uvs;           // [n_attr][3][2]
    const uint2*    irradiance;    // RGBA16F atlas, extents in d
    const uint32_t* depth;         // RG16F atlas, extents in d
    // SURFACE: a small attribute set (SceneShading's arrays, with tex_table / tex_data above) and one instance matrix
    const float*    positions;     // [n_tris][3][3]
    const float*    normals;       // [n_tris][3][3]
    const float*    tangents;      // [n_tris][3][3]
    const float*    tri_uvs;       // [n_tris][3][2]
    const uint32_t* tri_material;  // [n_tris]
    const float*    materials;     // [n_mats][8]
    const int32_t*  mat_tex;       // [n_mats][6]
    const float*    inst_m;        // column-major 16 floats
    int32_t         cube_size, pre_size, pre_levels, lut_size, n_tex, n_attr, n_tris, n_mats;
    hr_ddgi_uniforms d;
    hr_light        light;
};
static_assert(sizeof(ShadingTables) == 17 * 8 + 8 * 4 + 88 + 64, "ShadingTables layout");
