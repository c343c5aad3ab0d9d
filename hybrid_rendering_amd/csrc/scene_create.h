// What the scene creators share (api.hip hr_scene_create[_deformable], instances.hip hr_scene_create_instanced, instances_shared.hip
// hr_scene_create_instanced_shared[_deformable] and hr_instanced_scene_footprint).  Host code only.  `who` is the call's name as its messages spell it.
#pragma once
#include "hr_internal.h"
#include <cstring>
#include <new>

namespace hr {

#define HR_TRY(expr) do { const hr_status st_ = (expr); if (st_ != HR_OK) return st_; } while (0)

// No exception crosses the C ABI: the builder's and the staging vectors' allocation failures become HR_ERR_OUT_OF_MEMORY.
template <class F>
hr_status guarded(const char* call, F&& body)
{
    try
    {
        return body();
    }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
    catch (const std::exception& e)   // nothing else is expected
    {
        set_last_error(std::string(call) + ": " + e.what());
        return HR_ERR_UNSUPPORTED;
    }
}

// allocate and fill, synchronously (creation is not a hot path)
inline hr_status upload(DevBuf& buf, const void* src, size_t bytes)
{
    HR_TRY(buf.alloc(bytes));
    if (bytes == 0) return HR_OK;
    const hipError_t e = hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) return HR_OK;
    set_last_error(std::string("hipMemcpy H2D failed: ") + hipGetErrorString(e));
    return HR_ERR_HIP;
}

// materials, and for a textured desc (hr_scene_desc or hr_instanced_scene_desc) mat_tex, one buffer of texels and a table { texel offset, width,
// height, 0 } per texture: sets n_materials and has_textures.  The texture coordinates and tangents are the caller's (per triangle or per mesh).
template <class Desc>
hr_status stage_materials(hr_scene* s, const Desc* d, const char* who)
{
    HR_TRY(upload(s->materials, d->materials, d->materials ? (size_t)d->n_materials * 32 : 0));
    s->n_materials = d->materials ? d->n_materials : 0;
    if (!(d->material_textures && d->materials && d->n_textures > 0 && d->textures)) return HR_OK;
    std::vector<uint32_t> table;
    std::vector<uint8_t>  texels;
    for (int i = 0; i < d->n_textures; i++)
    {
        const hr_texture& t = d->textures[i];
        if (!t.rgba8 || t.width <= 0 || t.height <= 0) { set_last_error(std::string(who) + ": empty texture"); return HR_ERR_INVALID_ARG; }
        table.insert(table.end(), { (uint32_t)(texels.size() / 4), (uint32_t)t.width, (uint32_t)t.height, 0u });
        texels.insert(texels.end(), t.rgba8, t.rgba8 + (size_t)t.width * t.height * 4);
    }
    for (int i = 0; i < d->n_materials * 4; i++)
        if (d->material_textures[(i / 4) * 6 + (i % 4)] >= d->n_textures) { set_last_error(std::string(who) + ": material texture index out of range"); return HR_ERR_INVALID_ARG; }
    s->mat_albedo_host.resize((size_t)d->n_materials);   // what hr_scene_set_alpha_cutoffs validates against (cutout.hip)
    for (int m = 0; m < d->n_materials; m++) s->mat_albedo_host[(size_t)m] = d->material_textures[m * 6];
    HR_TRY(upload(s->mat_tex, d->material_textures, (size_t)d->n_materials * 24));
    HR_TRY(upload(s->tex_table, table.data(), table.size() * 4));
    HR_TRY(upload(s->tex_data, texels.data(), texels.size()));
    s->has_textures = true;
    return HR_OK;
}

// every triangle's material index is dereferenced by the hit shading (shading.h surface_at: materials[m * 8], mat_tex[m * 6]); -1: all in range
inline int first_bad_material(const uint32_t* tri_material, int n_tris, int n_materials)
{
    for (int i = 0; i < n_tris; i++)
        if (tri_material[i] >= (uint32_t)n_materials) return i;
    return -1;
}

// ---- instanced descs (instances.hip) -----------------------------------------------------------------------------------------------------------
// the attributes ALL meshes of a desc carry, concatenated in mesh order (an attribute some mesh lacks is dropped; normals and materials refuse that)
struct MeshAttributes
{
    bool                  normals = true, material = true, uvs = true, tangents = true;
    size_t                n_tris = 0;
    std::vector<float>    pos, nor, uv, tan;
    std::vector<uint32_t> mat;
};
hr_status mesh_attributes(const hr_instanced_scene_desc* d, const char* who, MeshAttributes& ma);

hr_status validate_instances(const hr_instanced_scene_desc* d, const char* who);   // mesh_idx in range, matrices finite
hr_status validate_desc(const hr_instanced_scene_desc* d, const char* who);        // the desc's counts and pointers, then validate_instances

struct MeshTrees
{
    std::vector<BuiltBVH>         blas;
    std::vector<int>              depth;        // per mesh: deepest node below the root (root = 0)
    std::vector<std::vector<int>> node_depth;   // per mesh, per node
};
// flags (or null): meshes that may deform are built without spatial splits (hr_scene_create_instanced_shared_deformable).  want_cells: the
// object-space cell of every leaf slot, 48 floats per node (the private-copy kind's refit cuts its leaves to them)
void build_mesh_trees(const hr_instanced_scene_desc* d, MeshTrees& mt, bool want_cells, const uint8_t* flags = nullptr);
// the host-side fields both kinds of instanced scene keep per instance and per mesh (what instanced_scene_boxes reads)
void fill_instances(hr_scene* s, const hr_instanced_scene_desc* d, const MeshTrees& mt);

// One 8-wide node out of the binary SAH tree `bin` (top_level_binary): the child of largest half area is opened until eight stand (instance leaves
// cannot be opened; ties go to the earlier child).  Returns their count; `axis`: the longest axis of the node's box, ties to the lower one —
// the walk's near-to-far hint (bvh.h), which the callers sort children along
int top_level_children(const std::vector<BinNode>& bin, int node, int kids[8], int& axis);
inline bool bin_before(const std::vector<BinNode>& bin, int axis, int x, int y)
{
    return (double)bin[(size_t)x].lo[axis] + bin[(size_t)x].hi[axis] < (double)bin[(size_t)y].lo[axis] + bin[(size_t)y].hi[axis];
}

} // namespace hr
