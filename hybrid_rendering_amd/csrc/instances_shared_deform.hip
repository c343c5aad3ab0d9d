// Deforming meshes inside a shared instanced scene (hr_scene_create_instanced_shared_deformable / hr_scene_update_meshes /
// hr_scene_mesh_refit_cost): instances_shared.hip (one object-space tree per mesh under a top level over the instances) with deform_refit.hip
// under it (new vertices, refit.h refit_node<false> over a split-free tree) — the reference's per-frame BLAS update followed by its TLAS re-build
// (main.cpp:74).  A flagged mesh is built without spatial splits; its levels of up to 32 nodes (half a wavefront) stay in the mesh's own workgroup.
//
// hr_scene_update_meshes, all on the caller's stream: deform_refit.hip's scatter into mesh_positions / mesh_normals and its refit of the updated
// meshes, kMaxUpdatesPerLaunch entries at a time; hr_scene_mesh_refit_cost is the engine's cost of one mesh.
// A deformed mesh changes its object-space bounds, and those feed every instance's world box, the top level and the `extent` of the walk's slack,
// all on the host.  With bounds == NULL the root boxes are copied to pinned memory and the call WAITS for that copy (the one stream wait); with
// bounds given nothing waits, and bounds that turn out too small are reported by hr_scene_mesh_refit_cost.  Too-small bounds can cost hits — the
// instance's world box no longer covers the mesh — but never an access outside the arrays: they only ever become box coordinates.
// Then instances_shared.hip shared_scene_host_tail: boxes, top level, records, two copies behind the refit launches on the same stream.
#include "deform_refit.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace hr;

namespace {

constexpr int kNarrowLevel = 32;            // levels of at most half a wavefront of nodes, from the root down to the first wider one, stay in the mesh's own workgroup

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

// the checks both calls share: a scene from hr_scene_create_instanced_shared_deformable and a flagged mesh of it
hr_status check_mesh(const hr_scene* scene, uint32_t mesh_idx, const char* call, const std::string& where)
{
    if (!scene) return bad(call, "scene is NULL");
    if (!scene->shared || !scene->deform) return bad(call, "not a scene from hr_scene_create_instanced_shared_deformable");
    const DeformRefit& sd = *scene->deform;
    if (mesh_idx >= (uint32_t)sd.flag.size()) return bad(call, where + "mesh_idx " + std::to_string(mesh_idx) + " >= n_meshes " + std::to_string(sd.flag.size()));
    if (!sd.flag[mesh_idx]) return bad(call, where + "mesh " + std::to_string(mesh_idx) + " was not flagged deformable when the scene was created");
    return HR_OK;
}

hr_status update_impl(hr_scene* s, const hr_mesh_update* up, int32_t n_updates, hipStream_t st)
{
    static const char* call = "hr_scene_update_meshes";
    if (!s) return bad(call, "scene is NULL");
    if (!s->shared || !s->deform) return bad(call, "not a scene from hr_scene_create_instanced_shared_deformable");
    if (n_updates < 0 || (n_updates > 0 && !up)) return bad(call, "updates is NULL or n_updates < 0");
    DeformRefit& sd = *s->deform;
    // everything is checked before anything is enqueued or any host state changes
    std::vector<int> active;
    for (int i = 0; i < n_updates; i++)
    {
        const hr_mesh_update& u = up[i];
        const std::string where = "updates[" + std::to_string(i) + "]: ";
        const hr_status cm = check_mesh(s, u.mesh_idx, call, where);
        if (cm != HR_OK) return cm;
        const int32_t nt = sd.n_tris[u.mesh_idx];
        if (u.first_tri < 0 || u.n_tris < 0 || (int64_t)u.first_tri + u.n_tris > (int64_t)nt)
            return bad(call, where + "triangles [" + std::to_string(u.first_tri) + ", " + std::to_string((int64_t)u.first_tri + u.n_tris) + ") outside the mesh's " + std::to_string(nt));
        if (u.n_tris == 0) continue;
        if (!u.positions) return bad(call, where + "positions is NULL");
        if (u.normals && !s->has_normals) return bad(call, where + "normals given for a scene created without normals");
        if (u.bounds)
        {
            for (int k = 0; k < 6; k++) if (!std::isfinite(u.bounds[k])) return bad(call, where + "bounds are not finite");
            for (int k = 0; k < 3; k++) if (u.bounds[k] > u.bounds[3 + k]) return bad(call, where + "bounds have lo > hi");
        }
        active.push_back(i);
    }
    if (active.empty()) return HR_OK;
    HR_HIP(hipSetDevice(s->ctx->device));
    {
        const hr_status mr = shared_mirrors_refresh(s);   // a device instance update ran since: the host tail below needs its matrices (one wait)
        if (mr != HR_OK) return mr;
        const hr_status ws = instanced_scene_wait_uploads(s);   // the staging vectors of the host tail may still feed the previous call's copies
        if (ws != HR_OK) return ws;
    }
    // the last entry that names a mesh decides its bounds
    const size_t M = sd.flag.size();
    std::vector<const float*> mesh_bounds(M, nullptr);
    std::vector<uint8_t>      touched(M, 0);
    for (int i : active) { mesh_bounds[up[i].mesh_idx] = up[i].bounds; touched[up[i].mesh_idx] = 1; }
    for (size_t at = 0; at < active.size(); at += kMaxUpdatesPerLaunch)
    {
        const size_t n = std::min(active.size() - at, (size_t)kMaxUpdatesPerLaunch);
        DeformScatterEntry        entries[kMaxUpdatesPerLaunch];
        std::vector<uint32_t>     ms;
        std::vector<const float*> bs;
        for (size_t j = 0; j < n; j++)
        {
            const hr_mesh_update& u = up[active[at + j]];
            entries[j] = { u.positions, u.normals, u.mesh_idx, u.first_tri, u.n_tris };
            if (std::find(ms.begin(), ms.end(), u.mesh_idx) == ms.end()) { ms.push_back(u.mesh_idx); bs.push_back(mesh_bounds[u.mesh_idx]); }
        }
        deform_refit_scatter(s, entries, (int)n, (float*)s->mesh_positions.p, s->has_normals ? (float*)s->mesh_normals.p : nullptr, st);
        const hr_status e = deform_refit_enqueue(s, (Node8*)s->nodes.p, ms.data(), (int)ms.size(), bs.data(), st);
        if (e != HR_OK) return e;
    }
    bool measure = false;
    for (size_t m = 0; m < M; m++) measure = measure || (touched[m] && !mesh_bounds[m]);
    if (measure)
    {
        HR_HIP(hipMemcpyAsync(sd.root_box_host, sd.root_box.p, M * 32, hipMemcpyDeviceToHost, st));
        HR_HIP(hipStreamSynchronize(st));   // the one wait of this call: the host tail needs the new bounds
        sd.stream_waits++;
    }
    for (size_t m = 0; m < M; m++)
    {
        if (touched[m]) sd.cost_known[m] = 0;
        if (!touched[m] || mesh_bounds[m]) continue;
        for (int k = 0; k < 8; k++)   // non-finite vertices are the caller's responsibility; a box made of them never reaches the top level
            if (!std::isfinite(sd.root_box_host[m * 8 + k])) return bad(call, "mesh " + std::to_string(m) + " is not finite after the update (the scene's top level stands as it was)");
    }
    for (size_t m = 0; m < M; m++)
    {
        if (!touched[m]) continue;
        float b[6];
        if (mesh_bounds[m]) std::memcpy(b, mesh_bounds[m], 24);
        else
            for (int k = 0; k < 3; k++) { b[k] = sd.root_box_host[m * 8 + k]; b[3 + k] = sd.root_box_host[m * 8 + 4 + k]; }
        for (int k = 0; k < 3; k++)
        {
            s->mesh_bounds[m * 6 + k] = b[k]; s->mesh_bounds[m * 6 + 3 + k] = b[3 + k];
            s->shared_mesh_absmax[m * 3 + k] = std::max(std::fabs(b[k]), std::fabs(b[3 + k]));
        }
    }
    {
        const hr_status mu = shared_device_mesh_table_upload(s, st);   // a device instance update after this one sees the new bounds
        if (mu != HR_OK) return mu;
    }
    return shared_scene_host_tail(s, st, false);
}

} // namespace

hr_status hr::shared_deform_adopt(hr_scene* s, const std::vector<BuiltBVH>& blas, const int32_t* mesh_n_tris, const uint8_t* flags)
{
    std::vector<DeformMesh> meshes(blas.size());
    size_t n_tris_all = 0, n_refs = 0;
    for (size_t k = 0; k < blas.size(); k++)   // the meshes' references and attributes are concatenated in mesh order (instances_shared.hip)
    {
        meshes[k] = { &blas[k], s->shared_mesh_root[k], (uint32_t)n_refs, (uint32_t)n_tris_all, mesh_n_tris[k], s->shared_mesh_pad[k], flags && flags[k], kNarrowLevel };
        n_refs += blas[k].tris.size();
        n_tris_all += (size_t)mesh_n_tris[k];
    }
    return deform_refit_adopt(s, meshes, "hr_scene_create_instanced_shared_deformable");
}

extern "C" {

hr_status hr_scene_update_meshes(hr_scene* scene, const hr_mesh_update* updates, int32_t n_updates, void* stream)
{
    try
    {
        return update_impl(scene, updates, n_updates, (hipStream_t)stream);
    }
    catch (const std::bad_alloc&)
    {
        set_last_error("hr_scene_update_meshes: host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
}

hr_status hr_scene_mesh_refit_cost(const hr_scene* scene, uint32_t mesh_idx, float* ratio)
{
    static const char* call = "hr_scene_mesh_refit_cost";
    const hr_status cm = check_mesh(scene, mesh_idx, call, "");
    if (cm != HR_OK) return cm;
    if (!ratio) return bad(call, "ratio is NULL");
    hr_scene* s = const_cast<hr_scene*>(scene);
    DeformRefit& sd = *s->deform;
    HR_HIP(hipSetDevice(s->ctx->device));
    HR_HIP(hipDeviceSynchronize());
    uint32_t outside = 0;
    HR_HIP(hipMemcpy(&outside, (const uint32_t*)sd.outside.p + mesh_idx, 4, hipMemcpyDeviceToHost));
    if (outside) return bad(call, "the bounds given with the last hr_scene_update_meshes do not contain mesh " + std::to_string(mesh_idx));
    return deform_refit_cost(s, mesh_idx, ratio);
}

hr_status hr_scene_update_meshes_stats(const hr_scene* scene, int64_t* level_launches, int64_t* top_launches, int64_t* stream_waits)
{
    if (!scene || !scene->shared || !scene->deform) return bad("hr_scene_update_meshes_stats", "not a scene from hr_scene_create_instanced_shared_deformable");
    if (level_launches) *level_launches = scene->deform->level_launches;
    if (top_launches) *top_launches = scene->deform->top_launches;
    if (stream_waits) *stream_waits = scene->deform->stream_waits;
    return HR_OK;
}

hr_status hr_scene_read_instance_records(const hr_scene* scene, void* records_out)
{
    if (!scene || !scene->shared || !records_out) return bad("hr_scene_read_instance_records", "not a shared instanced scene, or records_out is NULL");
    HR_HIP(hipSetDevice(scene->ctx->device));
    HR_HIP(hipDeviceSynchronize());
    HR_HIP(hipMemcpy(records_out, scene->inst_shared.p, (size_t)scene->n_instances * sizeof(InstanceShared), hipMemcpyDeviceToHost));
    return HR_OK;
}

} // extern "C"
