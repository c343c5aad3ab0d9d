// Deforming meshes inside a shared instanced scene (hr_scene_create_instanced_shared_deformable / hr_scene_update_meshes /
// hr_scene_mesh_refit_cost): the composition of instances_shared.hip (one object-space tree per mesh under a top level over the instances) and
// deform.hip (new vertices, refit.h refit_node<false> over a split-free tree) — the reference's per-frame BLAS update followed by its TLAS re-build
// (main.cpp:74).  A flagged mesh is built without spatial splits, so every finite triangle has ONE reference and a leaf's box is the bounds of its
// triangles plus the pad of that mesh's builder.
//
// hr_scene_update_meshes, all on the caller's stream, in this order (entries are taken kMaxUpdatesPerLaunch at a time):
//   k_shared_deform_scatter    one launch for all entries: one thread per updated triangle writes the 36 vertex bytes of its reference (prim and
//                              the padding words stand), the mesh's rows of mesh_positions and, when given, of mesh_normals
//   k_shared_deform_refit      level d of ALL updated meshes in one launch, deepest level first: the launch count follows the deepest updated
//                              mesh, not the number of meshes.  Only levels wider than kNarrowLevel nodes come here.
//   k_shared_deform_refit_top  one launch, one workgroup per updated mesh: the narrow levels near its root, a barrier between levels, then the
//                              refitted root box to root_box[mesh] and, when the caller gave bounds, whether they contain it to outside[mesh]
//                              (plain vector stores)
// Launch boundaries and workgroup barriers are the only ordering between levels (the per-XCD L2s are not coherent: see the header of instances.hip).
// Every workgroup stores the sum of its nodes' half areas in a slot of its own; hr_scene_mesh_refit_cost adds a mesh's slots in index order, so
// unchanged vertices give exactly 1.0.
// A deformed mesh changes its object-space bounds, and those feed every instance's world box, the top level and the `extent` of the walk's slack,
// all on the host.  With bounds == NULL the root boxes are copied to pinned memory and the call WAITS for that copy (the one stream wait); with
// bounds given nothing waits, and bounds that turn out too small are reported by hr_scene_mesh_refit_cost.  Too-small bounds can cost hits — the
// instance's world box no longer covers the mesh — but never an access outside the arrays: they only ever become box coordinates.
// Then instances_shared.hip shared_scene_host_tail: boxes, top level, records, two copies behind the refit launches on the same stream.
#include "hr_internal.h"
#include "refit.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace hr;

namespace {

constexpr int kMaxUpdatesPerLaunch = 64;    // entries (so meshes) one set of launches takes: the tables travel as kernel arguments
constexpr int kNarrowLevel = 32;            // levels of at most half a wavefront of nodes, from the root down to the first wider one, stay in the mesh's own workgroup
constexpr int kLevelStride = kMaxTraversalDepth + 2;

struct MeshDev
{
    uint32_t root, ref_base, tri_base;
    int32_t  n_tris, n_levels, d_top, partial_base;
    float    pad;
};
static_assert(sizeof(MeshDev) == 32, "MeshDev must be 32 bytes");

struct ScatterEntry { const float* positions; const float* normals; uint32_t mesh; int32_t first, count, block_first; };
struct ScatterArgs
{
    TriGPU*        tris;
    const int32_t* tri_ref;
    float*         positions;   // mesh_positions
    float*         normals;     // mesh_normals, or null
    const MeshDev* mesh;
    int            n;
    ScatterEntry   e[kMaxUpdatesPerLaunch];
};

__global__ __launch_bounds__(256) void k_shared_deform_scatter(ScatterArgs a)
{
    int j = 0;
    for (int i = 1; i < a.n; i++) if ((int)blockIdx.x >= a.e[i].block_first) j = i;
    const ScatterEntry& e = a.e[j];
    const int t = ((int)blockIdx.x - e.block_first) * 256 + (int)threadIdx.x;
    if (t >= e.count) return;
    const size_t g = (size_t)a.mesh[e.mesh].tri_base + (size_t)e.first + t;
    const float* p = e.positions + (size_t)t * 9;
    float v[9];
    for (int k = 0; k < 9; k++) v[k] = p[k];
    float* w = a.positions + g * 9;
    for (int k = 0; k < 9; k++) w[k] = v[k];
    const int32_t r = a.tri_ref[g];
    if (r >= 0)
    {
        TriGPU& d = a.tris[r];   // prim and the padding words stand
        d.v0[0] = v[0]; d.v0[1] = v[1]; d.v0[2] = v[2];
        d.v1[0] = v[3]; d.v1[1] = v[4]; d.v1[2] = v[5];
        d.v2[0] = v[6]; d.v2[1] = v[7]; d.v2[2] = v[8];
    }
    if (e.normals)
    {
        const float* n = e.normals + (size_t)t * 9;
        float*       o = a.normals + g * 9;
        for (int k = 0; k < 9; k++) o[k] = n[k];
    }
}

struct LevelArgs
{
    RefitArgs       r;          // list / count / pad unused: they differ per mesh
    const uint32_t* lists;
    const int32_t*  levels;
    const MeshDev*  mesh;
    double*         partials;
    int             d, n;
    uint32_t        idx[kMaxUpdatesPerLaunch];
    int32_t         block_first[kMaxUpdatesPerLaunch];
};

__global__ __launch_bounds__(64) void k_shared_deform_refit(LevelArgs a)
{
    int j = 0;
    for (int i = 1; i < a.n; i++) if ((int)blockIdx.x >= a.block_first[i]) j = i;
    const uint32_t m     = a.idx[j];
    const int32_t* row   = a.levels + (size_t)m * 2 * kLevelStride;
    const int      local = (int)blockIdx.x - a.block_first[j];
    const int      i     = row[a.d] + local * 64 + (int)threadIdx.x;
    double area = 0.0;
    if (i < row[a.d + 1])
    {
        RefitArgs r = a.r;
        r.pad = a.mesh[m].pad;
        area = refit_node<false>(r, a.lists[i]);
    }
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if (threadIdx.x == 0) a.partials[a.mesh[m].partial_base + row[kLevelStride + a.d] + local] = area;
}

struct TopArgs
{
    RefitArgs       r;
    const uint32_t* lists;
    const int32_t*  levels;
    const MeshDev*  mesh;
    double*         partials;
    float*          root_box;
    uint32_t*       outside;
    int             n;
    uint32_t        idx[kMaxUpdatesPerLaunch];
    uint64_t        has_bounds;                          // bit j: bounds[j] given
    float           bounds[kMaxUpdatesPerLaunch][6];
};

__global__ __launch_bounds__(256) void k_shared_deform_refit_top(TopArgs t)
{
    __shared__ double s_sum[4];
    const int      j   = (int)blockIdx.x;
    const uint32_t m   = t.idx[j];
    const MeshDev  md  = t.mesh[m];
    const int32_t* row = t.levels + (size_t)m * 2 * kLevelStride;
    RefitArgs r = t.r;
    r.pad = md.pad;
    double area = 0.0;
    for (int d = md.d_top; d >= 0; d--)
    {
        for (int i = row[d] + (int)threadIdx.x; i < row[d + 1]; i += 256) area += refit_node<false>(r, t.lists[i]);
        __threadfence_block();
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = area;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        t.partials[md.partial_base] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        const float* nb = r.node_box + (size_t)md.root * 8;
        float b[8];
        for (int k = 0; k < 8; k++) { b[k] = nb[k]; t.root_box[(size_t)m * 8 + k] = b[k]; }
        uint32_t out = 0u;
        if ((t.has_bounds >> j) & 1ull)
        {
            // the root box is the union of leaf boxes, each its triangles' bounds -/+ the pad in fp32: bounds that hold every vertex pass the
            // same subtraction / addition, which is monotonic, so exact bounds are never reported
            const float* g = t.bounds[j];
            for (int k = 0; k < 3; k++)
                if (!(b[k] >= g[k] - md.pad) || !(b[4 + k] <= g[3 + k] + md.pad)) out = 1u;
        }
        t.outside[m] = out;
    }
}

// the refit of the flagged meshes `ms` (at most kMaxUpdatesPerLaunch, distinct) into `nodes`; bounds[j]: the caller's bounds of ms[j], or null
hr_status enqueue_refit(hr_scene* s, Node8* nodes, const std::vector<uint32_t>& ms, const std::vector<const float*>& bounds, hipStream_t st)
{
    SharedDeform& sd = *s->shared_deform;
    RefitArgs r;
    r.nodes = nodes; r.tris = (const TriGPU*)s->tris.p; r.node_box = (float*)s->node_box.p; r.pad = 0.0f;
    r.cells = nullptr; r.node_inst = nullptr; r.inst = nullptr; r.dirty = nullptr; r.list = nullptr; r.count = 0;
    int deepest = 0;
    for (uint32_t m : ms) deepest = std::max(deepest, sd.n_levels[m]);
    for (int d = deepest - 1; d >= 0; d--)
    {
        LevelArgs a;
        a.r = r; a.lists = (const uint32_t*)sd.level_nodes.p; a.levels = (const int32_t*)sd.levels.p; a.mesh = (const MeshDev*)sd.mesh.p;
        a.partials = (double*)sd.partials.p; a.d = d; a.n = 0;
        int blocks = 0;
        for (uint32_t m : ms)
        {
            if (d >= sd.n_levels[m] || d <= sd.d_top[m]) continue;
            const int32_t* row = &sd.levels_host[(size_t)m * 2 * kLevelStride];
            const int count = row[d + 1] - row[d];
            if (count <= 0) continue;
            a.idx[a.n] = m; a.block_first[a.n] = blocks; a.n++;
            blocks += cdiv(count, 64);
        }
        if (a.n == 0) continue;
        hipLaunchKernelGGL(k_shared_deform_refit, dim3(blocks), dim3(64), 0, st, a);
        sd.level_launches++;
    }
    TopArgs t;
    t.r = r; t.lists = (const uint32_t*)sd.level_nodes.p; t.levels = (const int32_t*)sd.levels.p; t.mesh = (const MeshDev*)sd.mesh.p;
    t.partials = (double*)sd.partials.p; t.root_box = (float*)sd.root_box.p; t.outside = (uint32_t*)sd.outside.p;
    t.n = (int)ms.size(); t.has_bounds = 0;
    std::memset(t.bounds, 0, sizeof(t.bounds));
    for (size_t j = 0; j < ms.size(); j++)
    {
        t.idx[j] = ms[j];
        if (bounds[j]) { t.has_bounds |= 1ull << j; std::memcpy(t.bounds[j], bounds[j], 24); }
    }
    hipLaunchKernelGGL(k_shared_deform_refit_top, dim3((unsigned)ms.size()), dim3(256), 0, st, t);
    sd.top_launches++;
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status read_partials(hr_scene* s, uint32_t m, double* sum)
{
    SharedDeform& sd = *s->shared_deform;
    std::vector<double> part((size_t)sd.n_partials[m]);
    HR_HIP(hipMemcpy(part.data(), (const double*)sd.partials.p + sd.partial_base[m], part.size() * 8, hipMemcpyDeviceToHost));
    double a = 0.0;
    for (double v : part) a += v;
    *sum = a;
    return HR_OK;
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

// the checks both calls share: a scene from hr_scene_create_instanced_shared_deformable and a flagged mesh of it
hr_status check_mesh(const hr_scene* scene, uint32_t mesh_idx, const char* call, const std::string& where)
{
    if (!scene) return bad(call, "scene is NULL");
    if (!scene->shared_deform) return bad(call, "not a scene from hr_scene_create_instanced_shared_deformable");
    const SharedDeform& sd = *scene->shared_deform;
    if (mesh_idx >= (uint32_t)sd.flag.size()) return bad(call, where + "mesh_idx " + std::to_string(mesh_idx) + " >= n_meshes " + std::to_string(sd.flag.size()));
    if (!sd.flag[mesh_idx]) return bad(call, where + "mesh " + std::to_string(mesh_idx) + " was not flagged deformable when the scene was created");
    return HR_OK;
}

hr_status update_impl(hr_scene* s, const hr_mesh_update* up, int32_t n_updates, hipStream_t st)
{
    static const char* call = "hr_scene_update_meshes";
    if (!s) return bad(call, "scene is NULL");
    if (!s->shared_deform) return bad(call, "not a scene from hr_scene_create_instanced_shared_deformable");
    if (n_updates < 0 || (n_updates > 0 && !up)) return bad(call, "updates is NULL or n_updates < 0");
    SharedDeform& sd = *s->shared_deform;
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
        ScatterArgs a;
        a.tris = (TriGPU*)s->tris.p; a.tri_ref = (const int32_t*)sd.tri_ref.p; a.positions = (float*)s->mesh_positions.p;
        a.normals = s->has_normals ? (float*)s->mesh_normals.p : nullptr; a.mesh = (const MeshDev*)sd.mesh.p; a.n = (int)n;
        int blocks = 0;
        std::vector<uint32_t>     ms;
        std::vector<const float*> bs;
        for (size_t j = 0; j < n; j++)
        {
            const hr_mesh_update& u = up[active[at + j]];
            a.e[j] = { u.positions, u.normals, u.mesh_idx, u.first_tri, u.n_tris, blocks };
            blocks += cdiv(u.n_tris, 256);
            if (std::find(ms.begin(), ms.end(), u.mesh_idx) == ms.end()) { ms.push_back(u.mesh_idx); bs.push_back(mesh_bounds[u.mesh_idx]); }
        }
        hipLaunchKernelGGL(k_shared_deform_scatter, dim3(blocks), dim3(256), 0, st, a);
        const hr_status e = enqueue_refit(s, (Node8*)s->nodes.p, ms, bs, st);
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
    const size_t M = blas.size();
    s->shared_deform.reset(new SharedDeform());
    SharedDeform& sd = *s->shared_deform;
    sd.flag.assign(M, 0); sd.ref_base.assign(M, 0); sd.tri_base.assign(M, 0); sd.n_tris.assign(M, 0);
    sd.n_levels.assign(M, 0); sd.d_top.assign(M, -1); sd.partial_base.assign(M, 0); sd.n_partials.assign(M, 0);
    sd.cost_at_build.assign(M, 0.0); sd.cost_known.assign(M, 1); sd.cost_ratio.assign(M, 1.0);
    sd.levels_host.assign(M * 2 * kLevelStride, 0);
    size_t n_tris_all = 0, n_refs = 0;
    bool any = false;
    for (size_t k = 0; k < M; k++)
    {
        sd.flag[k] = flags && flags[k] ? 1 : 0;
        any = any || sd.flag[k];
        sd.ref_base[k] = (uint32_t)n_refs; n_refs += blas[k].tris.size();
    }
    for (size_t k = 0; k < M; k++)   // the meshes' attributes are concatenated in mesh order (instances_shared.hip)
    {
        sd.n_tris[k] = mesh_n_tris[k]; sd.tri_base[k] = (uint32_t)n_tris_all;
        n_tris_all += (size_t)mesh_n_tris[k];
    }
    if (!any) return HR_OK;
    std::vector<uint32_t> level_nodes;
    std::vector<int32_t>  tri_ref(n_tris_all, -1);
    std::vector<MeshDev>  mesh(M);
    std::memset(mesh.data(), 0, M * sizeof(MeshDev));
    int partials = 0;
    for (size_t k = 0; k < M; k++)
    {
        MeshDev& md = mesh[k];
        md.root = s->shared_mesh_root[k]; md.ref_base = sd.ref_base[k]; md.tri_base = sd.tri_base[k]; md.n_tris = sd.n_tris[k];
        md.pad = s->shared_mesh_pad[k]; md.d_top = -1;
        if (!sd.flag[k]) continue;
        const BuiltBVH& b = blas[k];
        const size_t n_nodes = b.nodes.size();
        std::vector<int> depth(n_nodes, 0);   // children follow their parent in the builder's breadth-first order
        int max_depth = 0;
        for (size_t j = 0; j < n_nodes; j++)
            for (int c = 0; c < (b.nodes[j].counts & 15); c++) { depth[(size_t)b.nodes[j].child_base + c] = depth[j] + 1; max_depth = std::max(max_depth, depth[j] + 1); }
        const int n_levels = max_depth + 1;
        if (n_levels + 1 > kLevelStride) { set_last_error("hr_scene_create_instanced_shared_deformable: a mesh tree deeper than the traversal stack"); return HR_ERR_UNSUPPORTED; }
        int32_t* row = &sd.levels_host[k * 2 * kLevelStride];
        std::vector<int32_t> width((size_t)n_levels, 0);
        for (size_t j = 0; j < n_nodes; j++) width[(size_t)depth[j]]++;
        row[0] = (int32_t)level_nodes.size();
        for (int d = 0; d < n_levels; d++) row[d + 1] = row[d] + width[(size_t)d];
        level_nodes.resize((size_t)row[n_levels]);
        {
            std::vector<int32_t> cur(row, row + n_levels);
            for (size_t j = 0; j < n_nodes; j++) level_nodes[(size_t)cur[(size_t)depth[j]]++] = md.root + (uint32_t)j;   // global node indices
        }
        int d_top = -1;
        while (d_top + 1 < n_levels && width[(size_t)d_top + 1] <= kNarrowLevel) d_top++;
        // slot 0: the one-workgroup launch; then the wide levels, deepest first
        int slot = 1;
        for (int d = n_levels - 1; d > d_top; d--) { row[kLevelStride + d] = slot; slot += cdiv(width[(size_t)d], 64); }
        sd.n_levels[k] = n_levels; sd.d_top[k] = d_top; sd.partial_base[k] = partials; sd.n_partials[k] = slot;
        md.n_levels = n_levels; md.d_top = d_top; md.partial_base = partials;
        partials += slot;
        for (size_t r = 0; r < b.tris.size(); r++)
        {
            const uint32_t prim = b.tris[r].prim;
            if (prim >= (uint32_t)sd.n_tris[k] || tri_ref[(size_t)sd.tri_base[k] + prim] >= 0)
            {
                set_last_error("hr_scene_create_instanced_shared_deformable: a triangle with more than one reference in a tree built without spatial splits");
                return HR_ERR_UNSUPPORTED;
            }
            tri_ref[(size_t)sd.tri_base[k] + prim] = (int32_t)(sd.ref_base[k] + r);
        }
    }
    const size_t n_nodes_all = (size_t)s->info.n_nodes;
    hr_status e;
    if ((e = sd.level_nodes.alloc(level_nodes.size() * 4)) != HR_OK) return e;
    if ((e = sd.levels.alloc(sd.levels_host.size() * 4)) != HR_OK) return e;
    if ((e = sd.mesh.alloc(M * sizeof(MeshDev))) != HR_OK) return e;
    if ((e = sd.tri_ref.alloc(tri_ref.size() * 4)) != HR_OK) return e;
    if ((e = sd.partials.alloc((size_t)partials * 8)) != HR_OK) return e;
    if ((e = sd.root_box.alloc(M * 32)) != HR_OK) return e;
    if ((e = sd.outside.alloc(M * 4)) != HR_OK) return e;
    if ((e = s->node_box.alloc(n_nodes_all * 32)) != HR_OK) return e;
    HR_HIP(hipHostMalloc((void**)&sd.root_box_host, M * 32, hipHostMallocDefault));
    std::memset(sd.root_box_host, 0, M * 32);
    HR_HIP(hipMemcpy(sd.level_nodes.p, level_nodes.data(), level_nodes.size() * 4, hipMemcpyHostToDevice));
    HR_HIP(hipMemcpy(sd.levels.p, sd.levels_host.data(), sd.levels_host.size() * 4, hipMemcpyHostToDevice));
    HR_HIP(hipMemcpy(sd.mesh.p, mesh.data(), M * sizeof(MeshDev), hipMemcpyHostToDevice));
    if (!tri_ref.empty()) HR_HIP(hipMemcpy(sd.tri_ref.p, tri_ref.data(), tri_ref.size() * 4, hipMemcpyHostToDevice));
    // one refit into a scratch copy of the nodes (the scene's own stay as built): node_box and the cost of every flagged tree as built
    DevBuf scratch;
    if ((e = scratch.alloc(n_nodes_all * sizeof(Node8))) != HR_OK) return e;
    HR_HIP(hipMemcpy(scratch.p, s->nodes.p, n_nodes_all * sizeof(Node8), hipMemcpyDeviceToDevice));
    std::vector<uint32_t> ms;
    for (size_t k = 0; k <= M; k++)
    {
        if (k < M && sd.flag[k]) ms.push_back((uint32_t)k);
        if (!ms.empty() && (k == M || ms.size() == (size_t)kMaxUpdatesPerLaunch))
        {
            if ((e = enqueue_refit(s, (Node8*)scratch.p, ms, std::vector<const float*>(ms.size(), nullptr), nullptr)) != HR_OK) return e;
            ms.clear();
        }
    }
    HR_HIP(hipStreamSynchronize(nullptr));
    for (size_t k = 0; k < M; k++)
        if (sd.flag[k] && (e = read_partials(s, (uint32_t)k, &sd.cost_at_build[k])) != HR_OK) return e;
    sd.level_launches = sd.top_launches = 0;
    return HR_OK;
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
    SharedDeform& sd = *s->shared_deform;
    HR_HIP(hipSetDevice(s->ctx->device));
    HR_HIP(hipDeviceSynchronize());
    uint32_t outside = 0;
    HR_HIP(hipMemcpy(&outside, (const uint32_t*)sd.outside.p + mesh_idx, 4, hipMemcpyDeviceToHost));
    if (outside) return bad(call, "the bounds given with the last hr_scene_update_meshes do not contain mesh " + std::to_string(mesh_idx));
    if (!sd.cost_known[mesh_idx])
    {
        double now = 0.0;
        const hr_status e = read_partials(s, mesh_idx, &now);
        if (e != HR_OK) return e;
        sd.cost_ratio[mesh_idx] = sd.cost_at_build[mesh_idx] > 0.0 ? now / sd.cost_at_build[mesh_idx] : 1.0;
        sd.cost_known[mesh_idx] = 1;
    }
    *ratio = (float)sd.cost_ratio[mesh_idx];
    return HR_OK;
}

hr_status hr_scene_update_meshes_stats(const hr_scene* scene, int64_t* level_launches, int64_t* top_launches, int64_t* stream_waits)
{
    if (!scene || !scene->shared_deform) return bad("hr_scene_update_meshes_stats", "not a scene from hr_scene_create_instanced_shared_deformable");
    if (level_launches) *level_launches = scene->shared_deform->level_launches;
    if (top_launches) *top_launches = scene->shared_deform->top_launches;
    if (stream_waits) *stream_waits = scene->shared_deform->stream_waits;
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
