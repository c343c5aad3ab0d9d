// Shared instanced scenes: every mesh's object-space 8-wide BVH is stored ONCE and walked on two levels (traverse2.h) — the reference's own scene
// model (scene_descriptor_set.glsl:30-34 Instance { mat4 model_matrix; uint mesh_idx; }, one BLAS per mesh, main.cpp:74 re-builds only the TLAS).
// Memory, creation and update cost O(sum of meshes + instances), against O(instances x mesh) of hr_scene_create_instanced's private copies.
//
//   nodes:        [ top level, root = 0, top_cap = max(1, instances) slots | mesh 0's tree | mesh 1's tree | ... ]
//   tris:         [ mesh 0's references | mesh 1's ... ]        object-space vertices, prim = mesh-local triangle index
//   inst_shared:  one 160-byte InstanceShared per LEAF of the top level, in leaf order (a top-level leaf slot's meta byte is (1 << 5) | j and
//                 the node's tri_base the record of its first leaf, so the walk's leaf mask names records directly)
//
// hr_scene_update_instances on such a scene is host work over the instances only: the inverse of every changed matrix (double), the instances'
// conservative world boxes, a refit of the top level's boxes (or a fresh SAH top level when the standing one has degraded: the same trigger as
// the private-copy kind), and two asynchronous copies — the top region of `nodes` and the records.  No vertex is transformed, no mesh node is
// touched.  Answers are those of the private-copy kind and of a flattened scene bit for bit: see traverse2.h for what keeps them so.
// Creation validates, builds the meshes' trees, fills the per-instance host fields and stages attributes, materials and textures through the
// functions the private-copy kind uses (scene_create.h, defined in instances.hip); the top level is collapsed by the same top_level_children.
#include "hr_internal.h"
#include "scene_create.h"
#include "instance_math.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>

using namespace hr;

namespace {

// ---- the top level: the binary SAH tree of instances.hip collapsed to 8-wide nodes whose leaves are instances --------------------------------------
struct SharedTop
{
    std::vector<hr_scene::SharedTopNode> nodes;
    std::vector<int32_t>                 leaf_inst;
    int                                  max_depth = 0;
};

void build_shared_top(const hr_scene* s, SharedTop& tl)
{
    const int I = s->n_instances;
    tl.nodes.clear(); tl.leaf_inst.clear(); tl.max_depth = 0;
    if (I == 1)
    {
        tl.nodes.push_back({ 0, 1, 0, 0, 0, 0 });
        tl.leaf_inst.push_back(0);
        return;
    }
    std::vector<BinNode> bin;
    bin.reserve((size_t)I * 2);
    std::vector<int> items((size_t)I);
    for (int i = 0; i < I; i++) items[(size_t)i] = i;
    const int root = top_level_binary(bin, items, I, s->inst_box.data());
    struct Q { int bin, depth; };
    std::vector<Q> queue { { root, 0 } };   // queue position = node slot
    for (size_t qi = 0; qi < queue.size(); qi++)
    {
        const Q q = queue[qi];
        int kids[8], ax;
        const int nk = top_level_children(bin, q.bin, kids, ax);
        int internal[8], ni = 0;
        hr_scene::SharedTopNode n { 0, 0, (int)queue.size(), (int)tl.leaf_inst.size(), ax, q.depth };
        for (int c = 0; c < nk; c++)
            if (bin[(size_t)kids[c]].inst < 0) internal[ni++] = kids[c];
            else { tl.leaf_inst.push_back(bin[(size_t)kids[c]].inst); n.n_leaves++; }
        // internal children sorted along the node's longest axis: the walk's near-to-far / far-to-near hint (bvh.h)
        std::stable_sort(internal, internal + ni, [&](int x, int y) { return bin_before(bin, ax, x, y); });
        n.n_internal = ni;
        for (int c = 0; c < ni; c++) queue.push_back({ internal[c], q.depth + 1 });
        if (ni) tl.max_depth = std::max(tl.max_depth, q.depth + 1);
        tl.nodes.push_back(n);
    }
}

// Boxes of a top level over the instances' current boxes, padded and quantised with the builder's rules (imath::top_node).  Returns the
// half-area sum of its nodes: what a re-build is judged by.
double refit_shared_top(const hr_scene* s, const SharedTop& tl, float pad, std::vector<Node8>& out)
{
    const size_t n = tl.nodes.size();
    out.assign((size_t)s->top_cap, Node8());
    std::memset(out.data(), 0, out.size() * sizeof(Node8));
    std::vector<float> box(n * 6);
    double sum = 0.0;
    for (size_t slot = n; slot-- > 0;)   // children sit behind their parent
    {
        const hr_scene::SharedTopNode& t = tl.nodes[slot];
        const int nc = t.n_internal + t.n_leaves;
        float clo[8][3], chi[8][3], lo[3], hi[3];
        for (int c = 0; c < nc; c++)
            for (int k = 0; k < 3; k++)
            {
                if (c < t.n_internal) { clo[c][k] = box[((size_t)t.child_base + c) * 6 + k]; chi[c][k] = box[((size_t)t.child_base + c) * 6 + 3 + k]; }
                else
                {
                    const float* b = &s->inst_box[(size_t)tl.leaf_inst[(size_t)t.leaf_base + (c - t.n_internal)] * 6];
                    clo[c][k] = b[k] - pad; chi[c][k] = b[3 + k] + pad;
                }
            }
        sum += imath::top_node(t, clo, chi, out[slot], lo, hi);
        for (int k = 0; k < 3; k++) { box[slot * 6 + k] = lo[k]; box[slot * 6 + 3 + k] = hi[k]; }
    }
    return sum;
}

// the deepest path of the two-level walk: one stack entry per level, plus the top level's entry parked at the instance boundary (traverse2.h)
bool shared_top_fits(const hr_scene* s, const SharedTop& tl) { return tl.max_depth + s->shared_mesh_depth + 2 < kMaxTraversalDepth; }

// one record: the matrix, its inverse (double, rounded once) and what the walk's slack needs (traverse2.h)
void fill_record(const hr_scene* s, int i, InstanceShared& r)
{
    const InstanceRec& h = s->inst_host[(size_t)i];
    const uint32_t     k = s->inst_mesh[(size_t)i];
    std::memset(&r, 0, sizeof(r));
    std::memcpy(r.m, h.m, 64);
    r.first_tri = h.first_tri; r.mesh_tri_base = h.mesh_tri_base; r.mesh_id = h.mesh_id; r.n_tris = h.n_tris;
    r.mesh_root = s->shared_mesh_root[k]; r.instance = (uint32_t)i;
    imath::record_terms(h.m, &s->shared_mesh_absmax[(size_t)k * 3], r.inv, r.inv_abs_row, &r.extent, &r.flags);
    r.flags |= (uint32_t)s->inst_mask[(size_t)i] << kInstanceMaskShift;   // the instance's mask goes wherever its record goes (bvh.h)
}

void adopt_shared_top(hr_scene* s, const SharedTop& tl)
{
    s->shared_top = tl.nodes;
    s->shared_leaf_inst = tl.leaf_inst;
    s->shared_leaf_of.assign((size_t)s->n_instances, 0);
    for (size_t l = 0; l < tl.leaf_inst.size(); l++) s->shared_leaf_of[(size_t)tl.leaf_inst[l]] = (int32_t)l;
    s->info.max_depth = tl.max_depth + 1 + s->shared_mesh_depth;
    s->fixed_shape = false;   // a host-built shape; top_cost_ratio is relative to the host's sum again (instances_shared_rebuild.hip)
    if (s->dev_update) s->dev_update->device_baseline = false;
}

float world_pad(const hr_scene* s) { return imath::pad_of_bounds(s->grid_lo, s->grid_hi); }

// deformable_call: hr_scene_create_instanced_shared_deformable (flags may still be null: no mesh can be updated then)
hr_status create_shared_impl(hr_ctx* ctx, const hr_instanced_scene_desc* d, hr_scene** out, bool deformable_call = false, const uint8_t* flags = nullptr)
{
    HR_CHECK_ARG(ctx && out);
    HR_TRY(validate_desc(d, deformable_call ? "hr_scene_create_instanced_shared_deformable" : "hr_scene_create_instanced_shared"));
    HR_CHECK_ARG(d->n_materials >= 0 && (d->materials || d->n_materials == 0));
    const int M = d->n_meshes, I = d->n_instances;
    const char* who = "hr_scene_create_instanced_shared";   // also what the deformable call's messages say from here on
    MeshAttributes ma;
    HR_TRY(mesh_attributes(d, who, ma));
    HR_HIP(hipSetDevice(ctx->device));

    MeshTrees mt;
    build_mesh_trees(d, mt, false, flags);
    std::unique_ptr<hr_scene> guard(new hr_scene());
    hr_scene* s = guard.get();
    s->ctx = ctx; s->shared = true;
    fill_instances(s, d, mt);
    s->top_cap = std::max(1, I);
    s->inst_mask.assign((size_t)I, 0xFFu);
    uint64_t n_nodes64 = (uint64_t)s->top_cap, n_refs64 = 0, n_tris64 = 0;
    for (int k = 0; k < M; k++) { n_nodes64 += mt.blas[(size_t)k].nodes.size(); n_refs64 += mt.blas[(size_t)k].tris.size(); }
    for (int i = 0; i < I; i++) n_tris64 += s->inst_host[(size_t)i].n_tris;
    if (n_tris64 >= (1ull << 31) || n_refs64 >= (1ull << 31)) { set_last_error("hr_scene_create_instanced_shared: more than 2^31 triangles"); return HR_ERR_UNSUPPORTED; }
    if (n_nodes64 >= (1ull << 23)) { set_last_error("hr_scene_create_instanced_shared: more than 2^23 BVH nodes"); return HR_ERR_UNSUPPORTED; }
    const size_t n_nodes = (size_t)n_nodes64;
    std::vector<Node8>  nodes(n_nodes);
    std::vector<TriGPU> tris((size_t)n_refs64);
    std::memset(nodes.data(), 0, n_nodes * sizeof(Node8));
    s->shared_mesh_root.resize((size_t)M);
    s->shared_mesh_absmax.assign((size_t)M * 3, 0.0f);
    s->shared_mesh_pad.resize((size_t)M);
    s->shared_mesh_depth = 0;
    size_t node_at = (size_t)s->top_cap, ref_at = 0;
    for (int k = 0; k < M; k++)
    {
        const BuiltBVH& b = mt.blas[(size_t)k];
        s->shared_mesh_root[(size_t)k] = (uint32_t)node_at;
        s->shared_mesh_pad[(size_t)k] = b.pad;
        s->shared_mesh_depth = std::max(s->shared_mesh_depth, mt.depth[(size_t)k]);
        if (d->meshes[k].n_tris > 0)
            for (int a = 0; a < 3; a++) s->shared_mesh_absmax[(size_t)k * 3 + a] = std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a]));
        for (size_t j = 0; j < b.nodes.size(); j++)
        {
            Node8 n = b.nodes[j];
            if (n.counts & 15) n.child_base += (uint32_t)node_at;
            n.tri_base += (uint32_t)ref_at;
            nodes[node_at + j] = n;
        }
        std::copy(b.tris.begin(), b.tris.end(), tris.begin() + ref_at);   // prim stays mesh-local
        node_at += b.nodes.size(); ref_at += b.tris.size();
    }
    instanced_scene_boxes(s);
    SharedTop tl;
    build_shared_top(s, tl);
    if (!shared_top_fits(s, tl)) { set_last_error("hr_scene_create_instanced_shared: top level + deepest mesh tree exceed the traversal stack"); return HR_ERR_UNSUPPORTED; }
    adopt_shared_top(s, tl);

    HR_TRY(upload(s->nodes, nodes.data(), n_nodes * sizeof(Node8)));
    HR_TRY(upload(s->tris, tris.data(), tris.size() * sizeof(TriGPU)));
    HR_TRY(upload(s->mesh_positions, ma.pos.data(), ma.n_tris * 36));
    if (ma.normals) { HR_TRY(upload(s->mesh_normals, ma.nor.data(), ma.n_tris * 36)); s->has_normals = true; }
    if (ma.material) { HR_TRY(upload(s->mesh_material, ma.mat.data(), ma.n_tris * 4)); s->has_material = true; }
    // textured materials, per mesh like the other attributes (same checks and layout as hr_scene_create_instanced)
    HR_TRY(stage_materials(s, d, who));
    if (s->has_textures)
    {
        if (ma.uvs) { HR_TRY(upload(s->mesh_uvs, ma.uv.data(), ma.n_tris * 24)); s->has_uvs = true; }
        if (ma.tangents) { HR_TRY(upload(s->mesh_tangents, ma.tan.data(), ma.n_tris * 36)); s->has_tangents = true; }
    }
    s->has_mesh_id = true;
    HR_TRY(s->inst_shared.alloc((size_t)I * sizeof(InstanceShared)));
    { static std::atomic<uint64_t> next_uid { 1ull << 41 }; s->uid = next_uid.fetch_add(1); }   // disjoint from the other kinds' counters
    if (const char* e = getenv("HR_TOP_LEVEL_REBUILD")) s->auto_rebuild = atoi(e) != 0;
    s->info.n_tris     = (int32_t)n_tris64;
    s->info.n_nodes    = (int32_t)n_nodes;
    s->info.node_bytes = n_nodes * sizeof(Node8);
    s->info.tri_bytes  = tris.size() * sizeof(TriGPU);
    // first update: the instances' own matrices, then wait (creation is synchronous like hr_scene_create)
    std::vector<float> mats((size_t)I * 16);
    for (int i = 0; i < I; i++) std::memcpy(&mats[(size_t)i * 16], d->instances[i].model_matrix, 64);
    s->top_area_at_build = -1.0;   // the first update records it
    HR_TRY(shared_device_tables_upload(s, nullptr, true));   // what hr_scene_update_instances_device reads
    HR_TRY(shared_scene_update(s, mats.data(), nullptr, false));
    HR_HIP(hipStreamSynchronize(nullptr));
    if (deformable_call)
    {
        std::vector<int32_t> mesh_n_tris((size_t)M);
        for (int k = 0; k < M; k++) mesh_n_tris[(size_t)k] = d->meshes[k].n_tris;
        HR_TRY(shared_deform_adopt(s, mt.blas, mesh_n_tris.data(), flags));
    }
    s->geometry_epoch = 0;
    *out = guard.release();
    return HR_OK;
}

hr_status footprint_impl(const hr_instanced_scene_desc* d, int32_t shared, hr_scene_info* info)
{
    HR_CHECK_ARG(info);
    HR_TRY(validate_desc(d, "hr_instanced_scene_footprint"));
    std::memset(info, 0, sizeof(*info));
    MeshTrees mt;
    build_mesh_trees(d, mt, false);
    hr_scene stub;
    fill_instances(&stub, d, mt);
    const int I = d->n_instances, M = d->n_meshes;
    uint64_t n_tris = 0, n_nodes = 0, n_refs = 0;
    std::vector<int> inst_depth((size_t)I);
    for (int i = 0; i < I; i++)
    {
        const BuiltBVH& b = mt.blas[stub.inst_mesh[(size_t)i]];
        n_tris += stub.inst_host[(size_t)i].n_tris;
        inst_depth[(size_t)i] = mt.depth[stub.inst_mesh[(size_t)i]];
        stub.max_rel_depth = std::max(stub.max_rel_depth, inst_depth[(size_t)i]);
        if (!shared) { n_nodes += b.nodes.size() - 1; n_refs += b.tris.size(); }
    }
    if (shared)
    {
        stub.top_cap = std::max(1, I);
        for (int k = 0; k < M; k++) { n_nodes += mt.blas[(size_t)k].nodes.size(); n_refs += mt.blas[(size_t)k].tris.size(); stub.shared_mesh_depth = std::max(stub.shared_mesh_depth, mt.depth[(size_t)k]); }
    }
    else
        stub.top_cap = I > 1 ? 2 * I : 1;
    n_nodes += (uint64_t)stub.top_cap;
    info->n_tris     = (int32_t)std::min<uint64_t>(n_tris, 0x7fffffffull);
    info->n_nodes    = (int32_t)std::min<uint64_t>(n_nodes, 0x7fffffffull);
    info->node_bytes = n_nodes * sizeof(Node8);
    info->tri_bytes  = n_refs * sizeof(TriGPU);
    const char* kind = shared ? "shared" : "private-copy";
    if (n_tris >= (1ull << 31) || n_refs >= (shared ? (1ull << 31) : (1ull << 26)))
    {
        set_last_error(std::string("hr_instanced_scene_footprint: a ") + kind + " scene of this desc holds " + std::to_string(n_refs) + " triangle references (limit " + (shared ? "2^31" : "2^26") + ")");
        return HR_ERR_UNSUPPORTED;
    }
    if (n_nodes >= (1ull << 23)) { set_last_error(std::string("hr_instanced_scene_footprint: more than 2^23 BVH nodes in a ") + kind + " scene"); return HR_ERR_UNSUPPORTED; }
    bool fits;
    if (shared)
    {
        instanced_scene_boxes(&stub);
        SharedTop tl;
        build_shared_top(&stub, tl);
        info->max_depth = tl.max_depth + 1 + stub.shared_mesh_depth;
        fits = shared_top_fits(&stub, tl);
    }
    else
    {
        info->max_depth = private_copy_top_depth(&stub, inst_depth);
        fits = info->max_depth + 1 < kMaxTraversalDepth;
    }
    for (int a = 0; a < 3; a++) { info->bounds_lo[a] = stub.grid_lo[a]; info->bounds_hi[a] = stub.grid_hi[a]; }
    info->box_pad = world_pad(&stub);
    if (!fits) { set_last_error(std::string("hr_instanced_scene_footprint: BVH depth of a ") + kind + " scene exceeds the traversal stack"); return HR_ERR_UNSUPPORTED; }
    return HR_OK;
}

} // namespace

bool hr::reject_shared_scene(const hr_scene* s, const char* pass)
{
    if (!s || !s->shared || s->two_level_passes) return false;
    set_last_error(std::string(pass) + ": a shared instanced scene (hr_scene_create_instanced_shared) is not supported by this pass yet; use hr_scene_create_instanced");
    return true;
}

bool hr::reject_shared_dev_switches(const hr_scene* s, const char* call, bool wanted)
{
    if (!s->shared || !wanted) return false;
    set_last_error(std::string(call) + ": trace statistics and developer switches are not available on a shared instanced scene");
    return true;
}

// matrices == nullptr: the standing ones (force_rebuild: hr_scene_rebuild_top_level)
hr_status hr::shared_scene_update(hr_scene* s, const float* matrices, hipStream_t st, bool force_rebuild)
{
    const int I = s->n_instances;
    const bool first = s->top_area_at_build < 0.0;
    bool any = first || force_rebuild || s->mirrors_stale;   // after a device update every instance counts as changed
    if (matrices)
        for (int i = 0; i < I; i++)
        {
            if (!finite_matrix(matrices + (size_t)i * 16)) { set_last_error("hr_scene_update_instances: model_matrices[" + std::to_string(i) + "] is not finite"); return HR_ERR_INVALID_ARG; }
            any = any || std::memcmp(s->inst_host[(size_t)i].m, matrices + (size_t)i * 16, 64) != 0;
        }
    if (!any) return HR_OK;
    HR_HIP(hipSetDevice(s->ctx->device));
    {
        const hr_status ms = shared_mirrors_refresh(s);   // a device update ran since: the matrices come back from the records (one wait)
        if (ms != HR_OK) return ms;
        const hr_status ws = instanced_scene_wait_uploads(s);   // the staging vectors below may still feed the previous call's copies
        if (ws != HR_OK) return ws;
    }
    if (matrices)
        for (int i = 0; i < I; i++) std::memcpy(s->inst_host[(size_t)i].m, matrices + (size_t)i * 16, 64);
    return shared_scene_host_tail(s, st, force_rebuild);
}

// the caller has waited for the previous call's uploads (instanced_scene_wait_uploads) and set the device
hr_status hr::shared_scene_host_tail(hr_scene* s, hipStream_t st, bool force_rebuild)
{
    const int I = s->n_instances;
    const bool first = s->top_area_at_build < 0.0;
    bool adopted = false;
    instanced_scene_boxes(s);
    s->info.box_pad = world_pad(s);
    for (int a = 0; a < 3; a++) { s->info.bounds_lo[a] = s->grid_lo[a]; s->info.bounds_hi[a] = s->grid_hi[a]; }   // conservative: no vertex is ever transformed here
    SharedTop cur;
    cur.nodes = s->shared_top; cur.leaf_inst = s->shared_leaf_inst;
    double area = refit_shared_top(s, cur, s->info.box_pad, s->top_nodes_host);
    // the top level is re-built when the instances have moved far enough for its boxes to overlap (instances.hip: the same trigger), or on demand
    if (I > 1 && (force_rebuild || (!first && s->auto_rebuild && area > s->rebuild_ratio * s->top_area_at_build)))
    {
        SharedTop fresh;
        build_shared_top(s, fresh);
        if (shared_top_fits(s, fresh))   // checked on EVERY re-build: a deeper top level than the stack can hold is never adopted
        {
            std::vector<Node8> fresh_nodes;
            const double fresh_area = refit_shared_top(s, fresh, s->info.box_pad, fresh_nodes);
            if (force_rebuild || fresh_area < 0.9 * area)
            {
                adopt_shared_top(s, fresh);
                s->top_nodes_host.swap(fresh_nodes);
                s->top_rebuilds++;
                area = fresh_area;
                adopted = true;
            }
        }
        s->top_area_at_build = area;   // adopted: the fresh one's; otherwise the spread is the new normal
    }
    if (first) s->top_area_at_build = area;
    s->shared_host.resize((size_t)I);
    for (int i = 0; i < I; i++) fill_record(s, i, s->shared_host[(size_t)s->shared_leaf_of[(size_t)i]]);
    if (adopted)
    {
        const hr_status us = shared_device_tables_upload(s, st, false);   // the device update refits the topology the host adopted
        if (us != HR_OK) return us;
    }
    HR_HIP(hipMemcpyAsync(s->nodes.p, s->top_nodes_host.data(), (size_t)s->top_cap * sizeof(Node8), hipMemcpyHostToDevice, st));
    HR_HIP(hipMemcpyAsync(s->inst_shared.p, s->shared_host.data(), (size_t)I * sizeof(InstanceShared), hipMemcpyHostToDevice, st));
    {
        const hr_status ms = instanced_scene_mark_uploads(s, st);
        if (ms != HR_OK) return ms;
    }
    if (s->dev_update) s->dev_update->boxes_current = false;   // the device's instance boxes are those of its own last update
    s->geometry_epoch++;
    return HR_OK;
}

extern "C" {

hr_status hr_scene_create_instanced_shared(hr_ctx* ctx, const hr_instanced_scene_desc* desc, hr_scene** out)
{
    return guarded("hr_scene_create_instanced_shared", [&] { return create_shared_impl(ctx, desc, out); });
}

hr_status hr_scene_create_instanced_shared_deformable(hr_ctx* ctx, const hr_instanced_scene_desc* desc, const uint8_t* deformable, hr_scene** out)
{
    return guarded("hr_scene_create_instanced_shared_deformable", [&] { return create_shared_impl(ctx, desc, out, true, deformable); });
}

int32_t hr_scene_is_shared(const hr_scene* scene) { return scene && scene->shared ? 1 : 0; }

// a host-side flag only: no device array and no answer of the scene depends on it
hr_status hr_scene_enable_two_level_passes(hr_scene* scene, int32_t enable)
{
    HR_CHECK_ARG(scene);
    if (!scene->shared) { set_last_error("hr_scene_enable_two_level_passes: not a shared instanced scene (hr_scene_create_instanced_shared)"); return HR_ERR_INVALID_ARG; }
    scene->two_level_passes = enable != 0;
    return HR_OK;
}
int32_t hr_scene_two_level_passes(const hr_scene* scene) { return scene && scene->shared && scene->two_level_passes ? 1 : 0; }

hr_status hr_instanced_scene_footprint(const hr_instanced_scene_desc* desc, int32_t shared, hr_scene_info* info)
{
    return guarded("hr_instanced_scene_footprint", [&] { return footprint_impl(desc, shared, info); });
}

} // extern "C"
