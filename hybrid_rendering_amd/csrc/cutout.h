// Alpha-tested cutout materials (hr_scene_set_alpha_cutoffs): the accept test every walk runs on a triangle that has passed the
// watertight test, when the kernel is a CUTOUT instantiation.  A hit the test rejects does not exist for the ray: it does not occlude, does not
// shorten the far limit, takes no part in the tie-break and is never cached.
//
// The test is keyed on the ATTRIBUTE index of the triangle — the original triangle index of a flat scene, mesh_tri_base + the mesh-local index of
// a shared one: what the hit shading indexes uvs and tri_material with — never on anything stored in TriGPU, so refits, deforms, instance updates
// and re-builds leave it alone.  `tab` is derived by the setter's kernel (cutout.hip k_cutout_table): per attribute index { albedo texture + 1,
// cutoff bits }, { 0, 0 } for a triangle of an opaque material, which then costs a CUTOUT walk one 8-byte load.
#pragma once
#include "device_math.h"

namespace hr {

// what cutout_accept reads, by value in the kernel arguments of a CUTOUT instantiation (unset and unread in every other)
struct CutoutView
{
    const uint2*    tab;         // per attribute index: x = albedo texture + 1 (0: opaque), y = the material's cutoff (float bits).  Null: every
                                 // hit is accepted — how a CUTOUT kernel that fires several ray classes treats the forced-opaque ones
    const float*    uvs;         // [n][3][2] by attribute index
    const uint4*    tex_table;   // per texture: texel offset, width, height
    const uint32_t* tex_data;    // RGBA8 texels
};

// The pinned sampler, the ONE body behind shading.h sample_texture (channels 0..3) and the alpha test (channel 3): texture(s_Textures[i], uv)
// in a ray-tracing stage — level 0, bilinear with fp32 weights at uv * size - 0.5, REPEAT addressing, UNORM8 texel = b / 255.  out[k] = channel C0 + k.
template <int C0, int NC>
HR_DEV void sample_texture_channels(const uint4* __restrict__ tex_table, const uint32_t* __restrict__ tex_data, int tex, float u, float v, float* out)
{
    const uint4 t  = tex_table[tex];
    const int   w  = (int)t.y, h = (int)t.z;
    const float px = u * (float)w - 0.5f, py = v * (float)h - 0.5f;
    const float fx0 = floorf(px), fy0 = floorf(py);
    const float fx = px - fx0, fy = py - fy0;
    // (int) of a float outside the int range saturates (v_cvt_i32_f32; NaN: 0), so the texel's neighbour is taken AFTER the wrap: `(int)fx0 + 1`
    // would overflow there.  For every index in range ((i mod w) + 1) mod w is (i + 1) mod w.
    int x0 = (int)fx0 % w, y0 = (int)fy0 % h;
    x0 = x0 < 0 ? x0 + w : x0; y0 = y0 < 0 ? y0 + h : y0;
    const int x1 = x0 + 1 == w ? 0 : x0 + 1, y1 = y0 + 1 == h ? 0 : y0 + 1;
    const uint32_t* base = tex_data + t.x;
    const uint32_t t00 = base[(size_t)y0 * w + x0], t10 = base[(size_t)y0 * w + x1], t01 = base[(size_t)y1 * w + x0], t11 = base[(size_t)y1 * w + x1];
#pragma unroll
    for (int c = C0; c < C0 + NC; c++)
    {
        const float a = __fdiv_rn((float)((t00 >> (8 * c)) & 0xffu), 255.0f), b = __fdiv_rn((float)((t10 >> (8 * c)) & 0xffu), 255.0f);
        const float e = __fdiv_rn((float)((t01 >> (8 * c)) & 0xffu), 255.0f), g = __fdiv_rn((float)((t11 >> (8 * c)) & 0xffu), 255.0f);
        const float top = a * (1.0f - fx) + b * fx, bot = e * (1.0f - fx) + g * fx;
        out[c - C0] = top * (1.0f - fy) + bot * fy;
    }
}

// q: the triangle's attribute index; u, v: the barycentrics of the watertight test.  The uv interpolation is shading.h surface_from's, bit for bit.
// false iff the hit is ignored: alpha < cutoff.
HR_DEV bool cutout_accept(const CutoutView& c, size_t q, float u, float v)
{
    if (c.tab == nullptr) return true;   // a kernel that fires several ray classes: this one is forced opaque (hr_scene_set_ray_class_opaque)
    const uint2 e = c.tab[q];
    if (e.x == 0u) return true;
    const float  b0 = 1.0f - u - v;
    const float* qu = c.uvs + q * 6;
    const float  tu = (qu[0] * b0 + qu[2] * u) + qu[4] * v;
    const float  tv = (qu[1] * b0 + qu[3] * u) + qu[5] * v;
    float a;
    sample_texture_channels<3, 1>(c.tex_table, c.tex_data, (int)(e.x - 1u), tu, tv, &a);   // sample_texture(albedo_tex[m], tu, tv)[3]
    return !(a < __uint_as_float(e.y));
}

} // namespace hr
