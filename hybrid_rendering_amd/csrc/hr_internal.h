// Internal host-side plumbing shared by the pass implementations: error mapping, device buffers,
// per-stage hipEvent profiling (the DW_SCOPED_SAMPLE analogue, e.g. ray_traced_shadows.cpp:102,974).
#pragma once
#include "../../include/hr_api.h"
#include "bvh.h"
#include "instance_math.h"
#include <hip/hip_runtime.h>
#include <memory>
#include <string>
#include <vector>

struct hr_deferred;   // hr_api_post.h

namespace hr {

void set_last_error(const std::string& s);

#define HR_HIP(expr)                                                                                              \
    do                                                                                                            \
    {                                                                                                             \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess)                                                                                     \
        {                                                                                                         \
            ::hr::set_last_error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
            return HR_ERR_HIP;                                                                                    \
        }                                                                                                         \
    } while (0)

#define HR_CHECK_ARG(cond)                                                                 \
    do                                                                                     \
    {                                                                                      \
        if (!(cond))                                                                       \
        {                                                                                  \
            ::hr::set_last_error(std::string("invalid argument: ") + #cond);               \
            return HR_ERR_INVALID_ARG;                                                     \
        }                                                                                  \
    } while (0)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// hr_environment's prefiltered chain: level l has size prefiltered_size >> l, and the last level still has a texel (CubeMap::fetch with S = 0 would
// clamp its texel to -1 and read in front of the level)
inline bool prefiltered_chain_ok(int size, int levels) { return size > 0 && levels > 0 && levels < 32 && (size >> (levels - 1)) > 0; }

// Profiler ranges under the REFERENCE's sample names (DW_SCOPED_SAMPLE: ray_traced_shadows.cpp:102,974,1043,1096,1147,1221, ray_traced_ao.cpp:100,
// 865,985,1034,1042,1091, ray_traced_reflections.cpp:109,999,1089,1145,1188,1262, ddgi.cpp:91,769,831,864,906,945, ...), so that a
// `rocprofv3 --marker-trace` of an integrated frame reads like the reference's profiler tree.  Off unless hr_set_markers() / HR_MARKERS asks:
// 1 = roctx (librocprofiler-sdk-roctx.so, dlopen'ed on first use), 2 = an in-process log (tests).  api.hip.
void        sample_push(const char* name);
void        sample_pop();
const char* sample_name_of_stage(const char* stage);   // StageProfiler stage -> the reference's label
bool        samples_on();
struct ScopedSample
{
    bool on;
    explicit ScopedSample(const char* name) : on(samples_on()) { if (on) sample_push(name); }
    ~ScopedSample() { if (on) sample_pop(); }
    ScopedSample(const ScopedSample&) = delete;
    ScopedSample& operator=(const ScopedSample&) = delete;
};
#define HR_SCOPED_SAMPLE(name) ::hr::ScopedSample hr_scoped_sample_(name)

// is per-stage event profiling switched on for this pass? (frame.hip: timing events cannot be captured into a hipGraph)
bool profiling_enabled(const hr_shadows* p);
bool profiling_enabled(const hr_ao* p);
bool profiling_enabled(const hr_ddgi* p);
bool profiling_enabled(const hr_reflections* p);
// deferred.hip: the context a composite pass was created on (probe_vis.hip draws onto the pass's output)
hr_ctx* deferred_ctx(const ::hr_deferred* p);
// instances.hip: brings info.bounds_* of an instanced scene up to date with its last update (synchronises the device when they lag)
hr_status instanced_scene_refresh_bounds(const hr_scene* scene);

// instances.hip, shared with instances_shared.hip: the binary SAH tree over instance boxes (full sweep along three axes) both kinds of top level
// are collapsed from, the instances' conservative world boxes (fills inst_box, grid_lo / grid_hi), the upload fence of an update, and the depth
// of the private-copy layout's deepest path for a host-only scene stub (n_instances, inst_host, inst_mesh, mesh_bounds, top_cap, max_rel_depth set)
struct BinNode { float lo[3], hi[3]; int left, right, inst; };
int       top_level_binary(std::vector<BinNode>& t, std::vector<int>& items, int n, const float* boxes);
void      instanced_scene_boxes(hr_scene* s);
hr_status instanced_scene_wait_uploads(hr_scene* s);
hr_status instanced_scene_mark_uploads(hr_scene* s, hipStream_t st);
int       private_copy_top_depth(hr_scene* stub, const std::vector<int>& mesh_depth_of_instance);
bool      finite_matrix(const float* m);
// instances_shared.hip.  HR_REJECT_SHARED: first statement (after the argument checks) of every pass that walks a shared scene only after
// hr_scene_enable_two_level_passes (the refusal is the published default of this API revision)
bool      reject_shared_scene(const hr_scene* s, const char* pass);
#define HR_REJECT_SHARED(scene, pass) do { if (::hr::reject_shared_scene(scene, pass)) return HR_ERR_UNSUPPORTED; } while (0)
// HR_REJECT_SHARED_DEV: the two-level walk has no instrumented or developer variants — a trace call that is asked for one (`wanted`) on a shared
// scene refuses, before anything is enqueued or any state of the pass changes
bool      reject_shared_dev_switches(const hr_scene* s, const char* call, bool wanted);
#define HR_REJECT_SHARED_DEV(scene, call, wanted) do { if (::hr::reject_shared_dev_switches(scene, call, wanted)) return HR_ERR_UNSUPPORTED; } while (0)
hr_status shared_scene_update(hr_scene* s, const float* matrices, hipStream_t st, bool force_rebuild);
// instances_shared.hip: the second half of an update, over the standing matrices and mesh_bounds / shared_mesh_absmax — the instances' boxes, the
// top level's refit (or re-build), the records, the two copies on `st` and geometry_epoch++ (hr_scene_update_instances and hr_scene_update_meshes)
hr_status shared_scene_host_tail(hr_scene* s, hipStream_t st, bool force_rebuild);
// instances_shared_update.hip.  shared_device_tables_upload: the device copies of the top level's topology (all = false) and, with all = true,
// of inst_mesh and the per-mesh table too — asynchronous copies on `st` out of the scene's standing host vectors, allocating at the first call.
// shared_device_mesh_table_upload: the per-mesh table alone (mesh_bounds / shared_mesh_absmax changed).  shared_mirrors_refresh: after a device
// update, one wait and a read-back of the records' matrices into inst_host (the slow path of every host call that follows a device update).
hr_status shared_device_tables_upload(hr_scene* s, hipStream_t st, bool all);
hr_status shared_device_mesh_table_upload(hr_scene* s, hipStream_t st);
hr_status shared_mirrors_refresh(hr_scene* s);
// instances_shared_deform.hip: what hr_scene_update_meshes needs, for a shared scene that holds the uploaded trees `blas` (flagged meshes built
// without spatial splits): deform_refit.h deform_refit_adopt over all meshes.  Synchronous, like creation.
hr_status shared_deform_adopt(hr_scene* s, const std::vector<BuiltBVH>& blas, const int32_t* mesh_n_tris, const uint8_t* flags);
// api.hip: hr_scene_create (deformable = false) and hr_scene_create_deformable (the builder runs without spatial splits, then deformable_scene_adopt)
hr_status scene_create_flat(hr_ctx* ctx, const hr_scene_desc* d, hr_scene** out, bool deformable);
// deform.hip: what a refit needs, for a scene that holds the uploaded tree `b` (deform_refit.h deform_refit_adopt of one mesh); the exact bounds of the last hr_scene_update_vertices, read back on demand
hr_status deformable_scene_adopt(hr_scene* s, const BuiltBVH& b);
hr_status deformable_scene_refresh_bounds(const hr_scene* scene);
// cutout.hip.  HR_REJECT_CUTOUT: the instrumented and developer variants of a trace (`wanted`) have no CUTOUT instantiation — they refuse a scene whose
// cutouts are enabled for the call's ray class, before anything is enqueued or any state of the pass changes; with every cutoff 0 they run as ever
bool      reject_cutout_dev_switches(const hr_scene* s, int ray_class, const char* call, bool wanted);
#define HR_REJECT_CUTOUT(scene, ray_class, call, wanted) do { if (::hr::reject_cutout_dev_switches(scene, ray_class, call, wanted)) return HR_ERR_UNSUPPORTED; } while (0)
// emission.hip.  HR_REJECT_EMISSION: the same for a scene whose emission is live (hr_scene_set_emission and some emitting material) — no EMISSIVE
// instantiation of the instrumented and developer variants exists
bool      reject_emission_dev_switches(const hr_scene* s, const char* call, bool wanted);
#define HR_REJECT_EMISSION(scene, call, wanted) do { if (::hr::reject_emission_dev_switches(scene, call, wanted)) return HR_ERR_UNSUPPORTED; } while (0)
// lights.hip.  HR_REJECT_LIGHTS: the same for a scene with a non-empty light list (hr_scene_set_lights)
bool      reject_lights_dev_switches(const hr_scene* s, const char* call, bool wanted);
#define HR_REJECT_LIGHTS(scene, call, wanted) do { if (::hr::reject_lights_dev_switches(scene, call, wanted)) return HR_ERR_UNSUPPORTED; } while (0)

struct DevBuf
{
    void*  p     = nullptr;
    size_t bytes = 0;
    hr_status alloc(size_t n)
    {
        free();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess)
        {
            set_last_error(std::string("hipMalloc(") + std::to_string(n) + ") failed: " + hipGetErrorString(e));
            p = nullptr;
            return e == hipErrorOutOfMemory ? HR_ERR_OUT_OF_MEMORY : HR_ERR_HIP;
        }
        // Every pass image starts as zeros: rows a pass never writes (a band's history apron before the first exchange, the other
        // half of a ping-pong pair) then read the same on every run and in every object, instead of whatever the allocator recycled.
        e = hipMemset(p, 0, n);
        if (e != hipSuccess)
        {
            set_last_error(std::string("hipMemset(") + std::to_string(n) + ") failed: " + hipGetErrorString(e));
            (void)hipFree(p);
            p = nullptr;
            return HR_ERR_HIP;
        }
        // hipMemset on device memory returns before the fill has run (it is queued on the NULL stream); a caller that renders straight away on
        // a hipStreamNonBlocking stream is not ordered after it.  Creation is not a hot path: wait here, so that "created" means "zeroed"
        // (hr_api.h: every hr_*_create returns with its images initialised)
        e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess)
        {
            set_last_error(std::string("hipStreamSynchronize after hipMemset failed: ") + hipGetErrorString(e));
            (void)hipFree(p);
            p = nullptr;
            return HR_ERR_HIP;
        }
        bytes = n;
        return HR_OK;
    }
    void free()
    {
        if (p) (void)hipFree(p);
        p     = nullptr;
        bytes = 0;
    }
    ~DevBuf() { free(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// a tightly packed image of `bpp` bytes per texel as an hr_*_image / hr_*_output view
inline void fill_view(hr_image_view* v, void* data, int w, int h, int bpp, hr_format f)
{
    v->data = data; v->width = w; v->height = h; v->row_pitch_bytes = w * bpp; v->format = f;
}

// What the refit of split-free trees under new vertices keeps (deform_refit.hip) for a scene from hr_scene_create_deformable (one flagged mesh:
// the scene) or hr_scene_create_instanced_shared_deformable.  Everything is indexed by mesh; an unflagged mesh has no levels, no partials and -1
// in tri_ref.
struct DeformRefit
{
    std::vector<uint8_t>  flag;                   // per mesh: may be updated
    std::vector<uint32_t> root, ref_base, tri_base;   // per mesh: its root in `nodes` / first reference in `tris` / first triangle in the attribute arrays
    std::vector<int32_t>  n_tris, n_refs;         // per mesh: triangles / references (a flagged mesh: one per triangle that was finite when built)
    std::vector<int32_t>  n_levels, d_top;        // per mesh: levels of its tree / deepest level the one-workgroup launch takes (-1: unflagged)
    std::vector<int32_t>  partial_base, n_partials;
    std::vector<double>   cost_at_build;
    std::vector<uint8_t>  cost_known;             // per mesh: cost_ratio is that of the last update (0: it lags until the slots are read back)
    std::vector<double>   cost_ratio;
    DevBuf   level_nodes;                         // the flagged meshes' level lists, GLOBAL node indices
    std::vector<int32_t> levels_host;             // per mesh two rows of kMaxTraversalDepth + 2 ints: offsets into level_nodes, first partial slot of the level
                                                  // (they reach the kernels in their arguments)
    DevBuf   tri_ref;                             // per mesh triangle (concatenated): global index of its one reference, -1: none (not finite when built)
    DevBuf   partials;                            // per refit workgroup: sum of its nodes' half areas (double)
    DevBuf   root_box;                            // per mesh 8 floats: the refitted root box (lo xyz, 0, hi xyz, 0)
    DevBuf   bounds_bits;                         // per mesh 6 words: ordered bits of the exact bounds of its finite references during an update,
                                                  // 0xffffffff x 3, 0 x 3 between updates (deform_refit.hip k_deform_bounds)
    DevBuf   outside;                             // per mesh one word: the bounds given with the last update do not contain the refitted root box
    float*   root_box_host = nullptr;             // pinned, per mesh 8 floats
    int64_t  level_launches = 0, top_launches = 0, stream_waits = 0;   // what the updates so far enqueued (hr_scene_update_meshes_stats)
    // the device re-deal of a mesh's triangles among its standing reference slots (deform_redeal.hip).  The host table is written with the tree
    // (deform_refit_adopt); the device buffers are allocated by the first re-deal, never after
    std::vector<int32_t> slot_of_rank_host;       // per flagged mesh, at ref_base[m]: its reference slots (global) in depth-first order of its tree
    std::vector<uint8_t> redeal_ok;               // per mesh: the table stands (the tree's leaves name each of its references once)
    bool     redeal_ready = false;
    DevBuf   rd_slot_of_rank;                     // slot_of_rank_host on the device
    DevBuf   rd_codes[2], rd_idx[2];              // per triangle of the largest flagged mesh: code / triangle, ping-pong of the radix sort; rd_idx[0]: the order
    DevBuf   rd_hist;                             // radix sort: per digit and workgroup, a count, then its exclusive prefix
    DevBuf   rd_tris;                             // per reference of the largest flagged mesh: the records in the new order, before they are copied back
    ~DeformRefit() { if (root_box_host) (void)hipHostFree(root_box_host); }
};

// What hr_scene_update_instances_device keeps (instances_shared_update.hip); allocated by the first call, never after
struct SharedDeviceUpdate
{
    DevBuf   inst_box;                            // per instance 6 floats: the world box of the last update
    DevBuf   node_box;                            // per top-level slot 6 floats (the per-depth path; the one-launch path keeps them in LDS)
    DevBuf   areas;                               // per top-level slot: its half area (double)
    DevBuf   status;                              // DeviceUpdateStatus
    void*    status_host = nullptr;               // pinned copy of `status`
    bool     status_stale = false;                // status_host lags the last update
    bool     given_bounds = false;                // the last update was given its bounds
    bool     captured = false;                    // an update was enqueued on a capturing stream: replays run it unseen
    hipStream_t last_stream = nullptr;            // of the last update enqueued
    double   area_at_build = 0.0;                 // the scene's top_area_at_build when the last update was enqueued
    int64_t  launches = 0, stream_waits = 0;
    // the device re-build of the top level (instances_shared_rebuild.hip); its buffers are allocated by the first re-build, never after
    bool     boxes_current = false;               // inst_box and the status block's bounds are those of the standing records (a host update clears it)
    bool     device_baseline = false;             // top_cost_ratio is relative to the status block's baseline (a host re-build clears it)
    float    threshold = 0.0f;                    // hr_scene_set_device_rebuild_threshold; 0: off
    bool     rebuild_ready = false;
    DevBuf   rb_codes[2], rb_idx[2];              // per instance: Morton code / instance index, ping-pong of the radix sort; rb_idx[0]: the sorted order
    DevBuf   rb_hist;                             // radix sort: per digit and workgroup, a count, then its exclusive prefix
    DevBuf   rb_records;                          // the records gathered into the new leaf order, before they are copied back
    int64_t  rebuild_launches = 0;
    ~SharedDeviceUpdate() { if (status_host) (void)hipHostFree(status_host); }
};

// Stage profiler: one event pair per named stage, recorded on the pass stream.
// Per-stage HIP-event timing on the launch stream.  Every stage keeps a RING of event pairs, one pair per profiled frame,
// so that a caller can leave profiling on over a whole timed region and read the per-kernel AVERAGE afterwards
// (bench.py: roofline.achieved) without synchronising inside it.  A new frame starts when begin_frame() is called or when a
// stage is begun for the second time in the current frame (stage-level callers).  collect() averages every frame recorded
// since the previous collect() and starts over.
struct StageProfiler
{
    static constexpr int kRing = 512;
    struct Stage
    {
        std::string             name;
        std::vector<hipEvent_t> ev0, ev1;   // created lazily, up to kRing pairs
        std::vector<long long>  stamp;      // epoch * 2^32 + frame of the recording in each slot
        uint64_t                bytes = 0;
        int                     last_frame = -1;   // last frame index this stage was recorded in
    };
    bool               enabled = false;
    std::vector<Stage> stages;
    int                frame = 0;        // frames started since the last collect()
    long long          epoch = 0;        // collect() calls so far
    bool               frame_open = false;

    int find_or_add(const char* name)
    {
        for (size_t i = 0; i < stages.size(); i++)
            if (stages[i].name == name) return (int)i;
        if (stages.size() >= HR_MAX_STAGES) return -1;
        stages.emplace_back();
        stages.back().name = name;
        return (int)stages.size() - 1;
    }
    void begin_frame()
    {
        if (frame_open) frame++;
        frame_open = false;
    }
    int  marker_depth = 0;           // ranges begin() opened and end() still has to close
    int begin(const char* name, hipStream_t s, uint64_t algorithmic_bytes)
    {
        if (samples_on()) { sample_push(sample_name_of_stage(name)); marker_depth++; }
        if (!enabled) return -1;
        int i = find_or_add(name);
        if (i < 0) return -1;
        Stage& st = stages[i];
        if (frame_open && st.last_frame == frame) frame++;   // the stage repeats: a new frame has begun
        frame_open = true;
        const int slot = frame % kRing;
        while ((int)st.ev0.size() <= slot)
        {
            hipEvent_t a, b;
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            st.ev0.push_back(a);
            st.ev1.push_back(b);
            st.stamp.push_back(-1);
        }
        st.stamp[slot] = (epoch << 32) + frame;
        st.bytes      = algorithmic_bytes;
        st.last_frame = frame;
        (void)hipEventRecord(st.ev0[slot], s);
        return i;
    }
    void end(int i, hipStream_t s)
    {
        if (marker_depth > 0) { sample_pop(); marker_depth--; }
        if (i >= 0) (void)hipEventRecord(stages[i].ev1[stages[i].last_frame % kRing], s);
    }
    void collect(hr_stage_times* out)
    {
        out->n_stages = 0;
        const int n_frames = frame + (frame_open ? 1 : 0);
        const int first    = n_frames > kRing ? n_frames - kRing : 0;   // older slots were overwritten
        for (Stage& st : stages)
        {
            double sum = 0.0;
            int    cnt = 0;
            for (int f = first; f < n_frames; f++)
            {
                const int slot = f % kRing;
                if (slot >= (int)st.ev0.size()) continue;
                if (st.stamp[slot] != (epoch << 32) + f) continue;   // this stage did not run in frame f
                float ms = 0.0f;
                if (hipEventSynchronize(st.ev1[slot]) != hipSuccess) continue;
                if (hipEventElapsedTime(&ms, st.ev0[slot], st.ev1[slot]) != hipSuccess) continue;
                sum += ms;
                cnt++;
            }
            if (st.last_frame < 0 || cnt == 0) continue;
            const int k     = out->n_stages++;
            out->name[k]    = st.name.c_str();
            out->ms[k]      = (float)(sum / cnt);
            out->bytes[k]   = st.bytes;
            st.last_frame   = -1;
        }
        frame = 0;
        frame_open = false;
        epoch++;
    }
    ~StageProfiler()
    {
        for (Stage& st : stages)
        {
            for (auto e : st.ev0) (void)hipEventDestroy(e);
            for (auto e : st.ev1) (void)hipEventDestroy(e);
        }
    }
};

} // namespace hr

struct hr_ctx
{
    int            device = 0;
    hipDeviceProp_t props;
};

struct hr_scene
{
    hr_ctx*       ctx = nullptr;
    hr::DevBuf    nodes, tris;
    hr::DevBuf    tri_normals, tri_material, tri_mesh_id, materials, positions; // shading data (by original triangle index)
    hr::DevBuf    tri_uvs, tri_tangents, mat_tex, tex_table, tex_data;          // textured materials (optional)
    bool          has_uvs = false, has_tangents = false, has_textures = false;
    hr_scene_info info;
    uint64_t      uid = 0;   // unique per hr_scene_create (a destroyed scene's device addresses may be handed out again): key of per-scene caches in the passes
    int           n_materials = 0;
    bool          has_normals = false, has_material = false, has_mesh_id = false;
    // ---- instanced scenes (instances.hip); n_instances == 0: a flattened scene from hr_scene_create.  `nodes` / `tris` / `positions` /
    // `tri_normals` are then REWRITTEN by hr_scene_update_instances (world space); the mesh_* arrays hold the object-space attributes the
    // hit shading interpolates (meshes concatenated), tri_instance / inst_records map a global triangle to them
    int           n_instances = 0;
    uint64_t      geometry_epoch = 0;   // bumped by every update: with `uid` the key of geometry-dependent caches of the passes (AO entry table)
    hr::DevBuf    inst_records, tri_instance, mesh_positions, mesh_normals, mesh_uvs, mesh_tangents, mesh_material;
    hr::DevBuf    level_nodes, node_box, bounds_bits, leaf_cells, node_inst, inst_dirty_dev;
    // the top level over the instance roots lives in the first `top_cap` node slots and can be RE-BUILT (host SAH over the instances' boxes, then
    // the slots, the level lists and everything above the subtrees are uploaded again): what a fixed top level loses after long motion
    int                   top_cap = 1;            // node slots reserved for top-level nodes + instance roots (2 x instances)
    std::vector<hr::Node8> inst_root_node;        // per instance: its subtree's root (topology fields final), wherever the top level puts it
    std::vector<float>    inst_root_cells;        // per instance: the 48 leaf-cell floats of that root
    std::vector<int32_t>  node_inst_host, node_rel_depth;   // per node: owning instance (-1 top level) / depth below the instance root
    std::vector<float>    inst_box;               // per instance: conservative world box (lo xyz, hi xyz) of the last update, host side
    std::vector<hr::Node8> top_nodes_host;        // upload staging, kept alive for the asynchronous copies
    std::vector<uint32_t> level_nodes_host;
    std::vector<int32_t>  inst_root_slot;
    std::vector<float>    top_cells_host;
    int           top_used = 1;
    bool          auto_rebuild = true;            // HR_TOP_LEVEL_REBUILD=0 switches the automatic re-build off (developer A/B)
    double        rebuild_ratio = 1.5;
    double        top_area_at_build = 0.0;        // sum of the top-level nodes' half areas when it was built: the re-build trigger compares against it
    int           top_rebuilds = 0;
    std::vector<uint32_t> inst_dirty;             // per instance: its matrix changed in the update being enqueued
    // The uploads of an update are asynchronous copies out of the host mirrors above (inst_host, inst_dirty, the top-level staging vectors):
    // `uploads_done` is recorded behind them, and the next call that rewrites a mirror waits for it first (instances.hip wait_uploads)
    hipEvent_t    uploads_done = nullptr;
    bool          uploads_pending = false;
    ~hr_scene()
    {
        if (uploads_done) (void)hipEventDestroy(uploads_done);
        if (mask_stage) (void)hipHostFree(mask_stage);
        if (cutoff_copied) (void)hipEventDestroy(cutoff_copied);
        if (cutoff_stage) (void)hipHostFree(cutoff_stage);
        if (em_copied) (void)hipEventDestroy(em_copied);
        if (em_stage) (void)hipHostFree(em_stage);
        if (lights_copied) (void)hipEventDestroy(lights_copied);
        if (lights_stage) (void)hipHostFree(lights_stage);
    }
    int           max_rel_depth = 0;              // deepest node below an instance root (a fresh top level must leave room for it)
    std::vector<int32_t>  level_offsets;          // level_nodes[level_offsets[d] .. level_offsets[d + 1]): the nodes of depth d
    std::vector<uint32_t> inst_mesh;              // per instance: mesh index
    std::vector<hr::InstanceRec> inst_host;       // host copy of inst_records (matrices of the last update)
    std::vector<float>    mesh_bounds;            // per mesh: object-space lo xyz, hi xyz
    float         grid_lo[3] = { 0, 0, 0 }, grid_hi[3] = { 0, 0, 0 };   // bounds a pass may read WITHOUT synchronising: exact for a flattened scene, the
                                                                         // host's conservative bounds (transformed mesh boxes) for an instanced one
    // ---- shared instanced scenes (instances_shared.hip): `nodes` = [ top level, top_cap slots | mesh 0's tree | mesh 1's ... ], `tris` = the meshes'
    // object-space references (prim = mesh-local triangle), inst_shared = one InstanceShared per top-level leaf
    bool          shared = false;
    bool          two_level_passes = false;       // hr_scene_enable_two_level_passes: AO, DDGI, reflections and the ground truth take the scene (default: they refuse it)
    hr::DevBuf    inst_shared;
    std::vector<hr::InstanceShared> shared_host;  // upload staging, in leaf order
    std::vector<int32_t>  shared_leaf_of;         // per instance: its leaf (= record) index
    using SharedTopNode = hr::SharedTopNode;     // instance_math.h
    std::vector<SharedTopNode> shared_top;        // per used top-level slot
    std::vector<int32_t>  shared_leaf_inst;       // per leaf: the instance
    std::vector<float>    shared_mesh_absmax;     // per mesh: max |p_k| over its bounds, per axis
    std::vector<uint32_t> shared_mesh_root;       // per mesh: node index of its root
    int           shared_mesh_depth = 0;          // deepest mesh tree (levels below its root)
    std::vector<float>    shared_mesh_pad;        // per mesh: the leaf pad its builder used
    // hr_scene_update_instances_device (instances_shared_update.hip): device copies of the top level's topology and of what a record is made
    // from, written at creation and wherever the host adopts a top level or new mesh bounds; `work` is allocated by the first device update
    hr::DevBuf    dev_top, dev_leaf_inst, dev_leaf_of, dev_inst_mesh, dev_mesh_tab;
    std::vector<int>      shared_depth_start;     // per top-level depth: its first slot (slots are breadth-first); one more entry: the slot count
    std::vector<uint32_t> shared_mesh_tri_base;   // per mesh: first triangle in the concatenated attribute arrays
    std::vector<float> mesh_tab_host;             // upload staging of dev_mesh_tab (per mesh 12 floats)
    std::unique_ptr<hr::SharedDeviceUpdate> dev_update;
    bool          fixed_shape = false;            // the top level has the shape of imath::fixed_top_node (a device re-build made it; a host re-build ends it)
    bool          order_replayed = false;         // a device re-build was CAPTURED: replays re-order the leaves where geometry_epoch cannot follow, so
                                                  // caches of the passes that hold top-level node indices (AO's entry table) are rebuilt at every use
    bool          mirrors_stale = false;          // a device update ran: inst_host / inst_box / top_nodes_host / shared_host lag the device
    // instance masks and per-ray-class cull masks (instances_shared_masks.hip).  The instance masks live in the records (bvh.h InstanceShared::flags);
    // inst_mask is the host's knowledge of them, by instance of the scene desc — stale (mirrors_stale) after hr_scene_set_instance_masks_device until
    // shared_mirrors_refresh reads the records back.  cull_mask is host state, read when a pass or query enqueues its launch
    std::vector<uint8_t>  inst_mask;
    uint32_t      cull_mask[HR_RAY_CLASS_COUNT] = { 0xFFu, 0xFFu, 0xFFu, 0xFFu, 0xFFu, 0xFFu };
    hr::DevBuf    mask_dev;                       // the host form's device staging, [n_instances] bytes; allocated by its first call
    uint8_t*      mask_stage = nullptr;           // ... and its pinned source, guarded by uploads_done like the other staging
    hipStream_t   mask_stream = nullptr;          // of the last hr_scene_set_instance_masks_device
    bool          masks_on_device = false;        // ... which a read-back has to wait for
    bool          masks_captured = false;         // ... enqueued on a capturing stream: replays rewrite the masks unseen
    // ---- alpha-tested cutout materials (cutout.hip, cutout.h).  alpha_cutoffs / class_opaque are host state, read when a pass or query
    // enqueues: a launch takes its CUTOUT instantiation iff cutout_enabled && !class_opaque[its ray class].  cutout_tab is keyed on the attribute
    // index (original triangle, or the mesh's offset + local triangle), so no update, refit or re-build of the scene touches it
    std::vector<float>    alpha_cutoffs;          // per material as last set; empty: never set (all opaque)
    bool          cutout_enabled = false;         // some cutoff is above 0
    int32_t       class_opaque[HR_RAY_CLASS_COUNT] = { 0, 0, 0, 0, 0, 0 };
    std::vector<int32_t>  mat_albedo_host;        // per material: its albedo texture (-1 none); filled at creation with mat_tex (scene_create.h), empty without textures
    hr::DevBuf    cutoff_dev, cutout_tab;         // [n_materials] floats; per attribute index { albedo texture + 1 or 0, cutoff bits }; allocated by the first setter call
    float*        cutoff_stage = nullptr;         // pinned source of the copy into cutoff_dev; the next call waits for cutoff_copied before it rewrites it
    hipEvent_t    cutoff_copied = nullptr;
    // ---- emissive materials (emission.hip, emission.h; DESIGN.md §7 "Emissive materials").  emission_enabled / emission_scale are host state, read when a pass or query
    // enqueues: a hit-shading launch takes its EMISSIVE instantiation iff emission_live().  The tables are keyed on the material, so no update of
    // the geometry touches them; allocated by the first setter call, never after
    bool          emission_enabled = false;
    float         emission_scale = 1.0f;
    std::vector<float>    emissive_host;          // [n_materials][3] as the host last set them (initially materials[m][5..7]); empty: no setter call yet
    std::vector<int32_t>  emissive_tex_host;      // [n_materials]: emissive texture, -1 none
    bool          emissive_on_device = false;     // hr_scene_set_emissive_device ran since the last host form: the host does not know the constants
    bool          emission_any = false;           // some material emits, as far as the host knows (emissive_on_device: assumed)
    hr::DevBuf    em_rgb, em_tex, em_inst;        // the tables of EmissionView; instanced kinds: per instance { first_tri, mesh_tri_base } + a sentinel (hr_scene_emission)
    float*        em_stage = nullptr;             // pinned source of the host forms' copies: [M][3] floats, then [M] int32; guarded by em_copied
    hipEvent_t    em_copied = nullptr;
    // ---- extra lights (lights.hip, lights.h; include/hr_lights.h).  The list is host state, read when a pass enqueues: a hit-shading launch takes
    // its LIGHTS instantiation iff lights_live().  The table of HR_MAX_LIGHTS records is allocated by the first setter call, never after
    std::vector<hr_light> lights_host;            // the list as the host last set it; its size is the count every launch passes
    hr::DevBuf    lights_dev;                     // [HR_MAX_LIGHTS] hr_light
    hr_light*     lights_stage = nullptr;         // pinned source of the host form's copy; guarded by lights_copied
    hipEvent_t    lights_copied = nullptr;
    // ---- deforming geometry (deform_refit.hip): trees built without spatial splits, refitted under new vertices through `deform` and node_box.
    // deform.hip: a flat scene (`deformable`); hr_scene_update_vertices rewrites `tris` / `positions` / `tri_normals`.  instances_shared_deform.hip: the
    // flagged meshes of a shared scene; hr_scene_update_meshes rewrites `tris` / `mesh_positions` / `mesh_normals`
    std::unique_ptr<hr::DeformRefit> deform;      // set by hr_scene_create_deformable and hr_scene_create_instanced_shared_deformable only
    bool          deformable = false;
    int64_t       redeals = 0, redeal_launches = 0;   // meshes re-dealt on the device / kernel launches enqueued for that so far (hr_scene_device_rebuild_counts);
                                                      // here and not in `deform`: a host rebuild replaces that
    mutable bool  bounds_stale = false;           // info.bounds_* lag the last update until hr_scene_get_info reads them back
    // ---- motion vectors (api.hip hr_scene_motion_begin_frame / hr_gbuffer_raycast_motion): the geometry as of the last begin_frame, indexed by
    // instance or by triangle, never by BVH reference — rebuilds, top-level re-builds and refits leave it alone
    bool          motion = false;                 // begin_frame has been called: the buffers below stand
    hr::DevBuf    prev_mats;                      // instanced kinds: [n_instances][16] model matrices, by instance index of the scene desc
    hr::DevBuf    prev_positions;                 // deformable: [n_tris][3][3] world; shared deformable: the object-space mesh_positions
};

namespace hr {
// the cull mask of a ray class in the place of the instance mask in a record's flags: what Scene2::cull holds
inline uint32_t cull_of(const hr_scene* s, int ray_class) { return (s->cull_mask[ray_class] & 0xFFu) << kInstanceMaskShift; }
// does a launch of `ray_class` over the scene take its CUTOUT instantiation?
inline bool cutout_on(const hr_scene* s, int ray_class) { return s->cutout_enabled && !s->class_opaque[ray_class]; }
// a -DHR_TRACE_DIVERGENCE build of the library (developer instrumentation, traverse.h)
#ifdef HR_TRACE_DIVERGENCE
constexpr bool kDivergenceBuild = true;
#else
constexpr bool kDivergenceBuild = false;
#endif
// does a hit-shading launch over the scene take its EMISSIVE instantiation?
inline bool emission_live(const hr_scene* s) { return s->emission_enabled && s->emission_any; }
// does a hit-shading launch over the scene take its LIGHTS instantiation?  n == 0 is off
inline bool lights_live(const hr_scene* s) { return !s->lights_host.empty(); }
inline Scene2 scene2_of(const hr_scene* s, int ray_class) { return Scene2 { (const Node8*)s->nodes.p, (const TriGPU*)s->tris.p, (const InstanceShared*)s->inst_shared.p, cull_of(s, ray_class) }; }
} // namespace hr
