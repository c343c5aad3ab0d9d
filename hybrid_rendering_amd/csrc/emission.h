// Emissive materials (DESIGN.md §7 "Emissive materials"; contract: include/hr_emission.h): the ONE text of the emission function, shared by the hit shaders of the
// EMISSIVE trace instantiations (ddgi.hip, reflections.hip, ground_truth.hip), the emissive image of the primary hits and the raw query
// (emission.hip).  tests/emission_reference.py restates it in float32 numpy.
//
// Keyed, like cutout.h, on the ATTRIBUTE index of the hit triangle — what surface_from indexes uvs and tri_material with — so refits, deforms,
// instance updates and re-builds leave it alone.  The per-material tables are the scene's own (hr_scene_set_emission allocates them).
#pragma once
#include "shading.h"

namespace hr {

// what emission_at reads, by value in the kernel arguments of an EMISSIVE instantiation (absent from every other)
struct EmissionView
{
    const float*   rgb;          // [n_materials][3]: the emissive constants as last set (hr_scene_set_emissive[_device]; initially materials[m][5..7])
    const int32_t* tex;          // [n_materials]: the emissive texture, an index into the scene's textures (-1: none)
    int            n_materials;
    float          scale;
};

// the attribute index of a hit: surface_at's, for each kind of scene
HR_DEV size_t attribute_index(const SceneShading& s, const HitRec& h)
{
    const InstanceRec* ir = s.tri_instance ? s.inst + s.tri_instance[h.prim] : nullptr;
    return ir ? (size_t)ir->mesh_tri_base + ((uint32_t)h.prim - ir->first_tri) : (size_t)h.prim;
}
HR_DEV size_t attribute_index(const SceneShading& s, const Hit2& h) { return (size_t)s.inst_shared[h.inst].mesh_tri_base + h.local; }

// E of a hit with barycentrics (hu, hv) on attribute triangle q.  false: the triangle's material does not emit and the caller performs NO add
// (a select, not an add of zero: "emission on, every material dark" is then bit-identical to "emission off", signed zeros included).
// A material emits iff its constant has a non-zero component or it has an emissive texture; the texture REPLACES the constant.  Two-sided.
HR_DEV bool emission_at(const EmissionView& e, const SceneShading& s, const size_t q, const float hu, const float hv, f3& E)
{
    const uint32_t mat = s.tri_material ? s.tri_material[q] : 0u;
    if (mat >= (uint32_t)e.n_materials) return false;   // a scene without materials: nothing emits
    const float*  c   = e.rgb + (size_t)mat * 3;
    const int32_t tex = e.tex[mat];
    f3 F = mk3(c[0], c[1], c[2]);
    if (!(tex >= 0 || F.x != 0.0f || F.y != 0.0f || F.z != 0.0f)) return false;
    if (tex >= 0)
    {
        float tu = 0.0f, tv = 0.0f;
        if (s.uvs)   // surface_from's expression
        {
            const float  b0 = 1.0f - hu - hv, b1 = hu, b2 = hv;
            const float* qu = s.uvs + q * 6;
            tu = (qu[0] * b0 + qu[2] * b1) + qu[4] * b2;
            tv = (qu[1] * b0 + qu[3] * b1) + qu[5] * b2;
        }
        float t[4];
        sample_texture(s, tex, tu, tv, t);
        F = mk3(t[0], t[1], t[2]);
    }
    E = mk3(e.scale * F.x, e.scale * F.y, e.scale * F.z);
    return true;
}
template <class Hit>
HR_DEV bool emission_at_hit(const EmissionView& e, const SceneShading& s, const Hit& h, f3& E) { return emission_at(e, s, attribute_index(s, h), h.u, h.v, E); }

} // namespace hr
