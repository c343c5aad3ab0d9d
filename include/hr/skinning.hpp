// C++ host shim over include/hr_skin.h, in the manner of passes.hpp: a skinned, morphed mesh posed on the GPU into the buffers a deformable
// scene's update takes.  (The reference has static meshes only and rebuilds its top level per frame, main.cpp:74: there is no class to mirror.)
//
//   a frame with an animated character, everything on one stream (cmd_buf)
//   ----------------------------------------------------------------------------------------------------------------------------------------
//   scene.motion_begin_frame(cmd_buf);                                     // the geometry as it stands becomes "previous frame"
//   skin.pose(cmd_buf, palette_device, morph_weights_device);              // or skin.pose_host(cmd_buf, palette, morph_weights)
//   scene.update_vertices(skin.positions(), skin.normals(), first_tri, skin.n_tris(), cmd_buf);
//       ... or, in a shared instanced scene:  hr_mesh_update u = skin.mesh_update(mesh_idx, box);  scene.update_meshes(&u, 1, cmd_buf);
//           with  float box[6];  skin.bounds(palette, morph_weights, box);  — no stream wait in the update
//   the passes
#pragma once
#include "../hr_skin.h"
#include "passes.hpp"
#include <vector>

namespace hr {

class Skin
{
public:
    // ctx may be omitted (Skin(desc)): a host-only skin for info() and bounds()
    Skin(Context& ctx, const hr_skin_desc& desc) { create(ctx.handle(), desc); }
    explicit Skin(const hr_skin_desc& desc) { create(nullptr, desc); }
    ~Skin() { hr_skin_destroy(m_skin); }
    Skin(const Skin&) = delete;
    Skin& operator=(const Skin&) = delete;

    // hr_skin_check_desc: HR_OK or HR_ERR_INVALID_ARG with the cause in hr_last_error(); never throws
    static hr_status check(const hr_skin_desc& desc) { return hr_skin_check_desc(&desc); }

    // device palette [n_joints][16] (and morph weights [n_targets], or nullptr): kernels only, capturable
    void pose(Stream cmd_buf, const float* joint_matrices_device, const float* morph_weights_device = nullptr)
    {
        hr::check(hr_skin_pose_device(m_skin, joint_matrices_device, morph_weights_device, cmd_buf), "Skin::pose");
    }
    // host palette: checked for finite values and staged through the skin's pinned buffer; not under capture
    void pose_host(Stream cmd_buf, const float* joint_matrices, const float* morph_weights = nullptr)
    {
        hr::check(hr_skin_pose(m_skin, joint_matrices, morph_weights, cmd_buf), "Skin::pose_host");
    }
    // device [n_tris][3][3], stable for the life of this object
    const float* positions() const { return m_positions; }
    const float* normals() const { return m_normals; }
    // the update of mesh `mesh_idx` of a shared instanced scene from this skin's buffers; bounds: host lo xyz hi xyz (bounds()), or nullptr: measured
    hr_mesh_update mesh_update(uint32_t mesh_idx, const float* bounds = nullptr, int32_t first_tri = 0) const
    {
        hr_mesh_update u;
        u.mesh_idx = mesh_idx; u.first_tri = first_tri; u.n_tris = m_info.n_tris;
        u.positions = m_positions; u.normals = m_normals; u.bounds = bounds;
        return u;
    }
    // conservative box of every position pose() writes for these arguments; false: the weights do not sum to 1 closely enough (pass nullptr as bounds)
    bool bounds(const float* joint_matrices, const float* morph_weights, float out[6]) const
    {
        const hr_status s = hr_skin_bounds(m_skin, joint_matrices, morph_weights, out);
        if (s == HR_ERR_UNSUPPORTED) return false;
        hr::check(s, "Skin::bounds");
        return true;
    }
    int32_t n_tris() const { return m_info.n_tris; }
    int32_t n_joints() const { return m_info.n_joints; }
    int32_t n_targets() const { return m_info.n_targets; }
    const hr_skin_info_data& info() const { return m_info; }
    void set_profiling(bool on) { hr::check(hr_skin_set_profiling(m_skin, on ? 1 : 0), "hr_skin_set_profiling"); }
    hr_stage_times stage_times()
    {
        hr_stage_times t;
        hr::check(hr_skin_get_stage_times(m_skin, &t), "hr_skin_get_stage_times");
        return t;
    }
    hr_skin* handle() const { return m_skin; }

private:
    void create(hr_ctx* ctx, const hr_skin_desc& desc)
    {
        hr::check(hr_skin_create(ctx, &desc, &m_skin), "hr_skin_create");
        hr::check(hr_skin_info(m_skin, &m_info), "hr_skin_info");
        if (ctx) hr::check(hr_skin_output(m_skin, &m_positions, &m_normals), "hr_skin_output");
    }
    hr_skin*          m_skin = nullptr;
    hr_skin_info_data m_info;
    const float*      m_positions = nullptr;
    const float*      m_normals = nullptr;
};

// hr_skin_pose_host: the contract on the CPU, positions then normals, [n_tris][3][3] each
inline void skin_pose_host(const hr_skin_desc& desc, const float* matrices, const float* morph_weights, std::vector<float>& positions, std::vector<float>& normals)
{
    const size_t n = desc.n_tris > 0 ? (size_t)desc.n_tris * 9 : 0;
    positions.assign(n, 0.0f);
    normals.assign(n, 0.0f);
    check(hr_skin_pose_host(&desc, matrices, morph_weights, positions.data(), normals.data()), "hr_skin_pose_host");
}

} // namespace hr
