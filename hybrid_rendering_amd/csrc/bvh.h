// Compressed 8-wide BVH: the software replacement for VK_KHR_acceleration_structure
// (reference call sites: main.cpp:74 build_tlas, common.cpp:355-521 initialize_for_ray_tracing).
//
// Node = 80 bytes (five 16-byte loads per lane):
//   [ 0] origin.xyz (f32), exponent bytes ex,ey,ez (biased like an fp32 exponent),
//        counts = n_internal | n_children << 4.  Slots 0..n_internal-1 are the internal children (slot i is node
//        child_base + i), slots n_internal..n_children-1 the leaves, the rest empty.
//   [16] child_base (index of first internal child), tri_base (index of first leaf triangle),
//        meta[8]: 0 = empty slot; internal: 0x10 (slot 0: 0x10 | the axis 0..2 the internal children are sorted along);
//                 leaf: (count << 5) | offset  (triangles tri_base+offset .. +count-1), count 1..4
//   [32] qlo.x[8] qlo.y[8]   [48] qlo.z[8] qhi.x[8]   [64] qhi.y[8] qhi.z[8]   (uint8 grid coords)
//   child box = origin + q * 2^(e-127), lo floored / hi ceiled => conservative.
// Triangle = 48 bytes: v0.xyz, prim | v1.xyz, 0 | v2.xyz, 0   (original vertex positions: the
// watertight test needs them unmodified for bit-reproducible hit decisions).
#pragma once
#include <stdint.h>
#include <vector>

namespace hr {

struct alignas(16) Node8
{
    float    ox, oy, oz;
    uint8_t  ex, ey, ez, counts;
    uint32_t child_base;
    uint32_t tri_base;
    uint8_t  meta[8];
    uint8_t  qlo[3][8];
    uint8_t  qhi[3][8];
};
static_assert(sizeof(Node8) == 80, "Node8 must be 80 bytes");

struct alignas(16) TriGPU
{
    float    v0[3];
    uint32_t prim;
    float    v1[3];
    uint32_t pad1;
    float    v2[3];
    uint32_t pad2;
};
static_assert(sizeof(TriGPU) == 48, "TriGPU must be 48 bytes");

// One instance of an instanced scene (instances.hip; scene_descriptor_set.glsl:30-34 Instance { mat4 model_matrix; uint mesh_idx; }): the
// hit shading maps a global triangle index to the mesh's object-space attributes and applies `m` (shading.h surface_at).
struct alignas(16) InstanceRec
{
    float    m[16];          // column-major object -> world
    uint32_t first_tri;      // global index of the instance's first triangle
    uint32_t mesh_tri_base;  // index of the mesh's first triangle in the concatenated per-mesh attribute arrays
    uint32_t mesh_id;        // GB3.z of the instance's pixels
    uint32_t n_tris;
};
static_assert(sizeof(InstanceRec) == 80, "InstanceRec must be 80 bytes");

// One instance of a SHARED instanced scene (instances_shared.hip, traverse2.h): the mesh's object-space tree is stored once, the walk enters it
// through `inv` and transforms the leaf triangles through `m` on the fly.  Records sit in the order of the top level's leaves.
struct alignas(16) InstanceShared
{
    float    m[16];          // column-major object -> world
    float    inv[9];         // column-major inverse of mat3(m) (host, double, rounded once)
    float    inv_abs_row[3]; // per object axis k: sum_j |inv(k, j)|
    float    extent;         // sum_j (|m(j, 3)| + sum_k |m(j, k)| max|p_k| over the mesh's bounds): the instance's world magnitude
    uint32_t flags;          // bit 0: no object-space culling (the matrix has no safe inverse).  Bits 8..15: the instance's mask
                             // (VkAccelerationStructureInstanceKHR::mask; 0xFF at creation, hr_scene_set_instance_masks): a ray walks into the
                             // instance iff mask & the ray's cull mask != 0.  It belongs to the INSTANCE: every writer of a record keeps it
    uint32_t first_tri;      // global index of the instance's first triangle
    uint32_t mesh_tri_base;  // index of the mesh's first triangle in the concatenated per-mesh attribute arrays
    uint32_t mesh_id;        // GB3.z of the instance's pixels
    uint32_t n_tris;
    uint32_t mesh_root;      // node index of the mesh tree's root
    uint32_t instance;       // index in the scene desc
    uint32_t pad[2];
};
static_assert(sizeof(InstanceShared) == 160, "InstanceShared must be 160 bytes");
constexpr uint32_t kInstanceMaskShift = 8u, kInstanceMaskBits = 0xFFu << kInstanceMaskShift;   // InstanceShared::flags
// what the two-level walk (traverse2.h) reads of a shared instanced scene
struct Scene2
{
    const Node8*          nodes;
    const TriGPU*         tris;
    const InstanceShared* inst;
    uint32_t              cull;    // the ray's cull mask (hr_scene_set_cull_mask, per ray class; 0xFF: every instance), SHIFTED to the place of the
                                   // instance mask in InstanceShared::flags: the walk's test is one AND (hr_internal.h scene2_of)
};

// deepest 8-wide tree the traversal's per-lane stack can walk (one entry per level, traverse.h LaneStack)
constexpr int kMaxTraversalDepth = 64;

struct BuiltBVH
{
    std::vector<Node8>  nodes;
    std::vector<TriGPU> tris;
    float               lo[3], hi[3];
    float               pad;
    int                 max_depth;
    int                 n_refs = 0;   // triangle references after splitting (== tris.size())
    // want_child_boxes (set before build_bvh8): child_boxes[(node * 8 + slot) * 6 ..] = lo xyz, hi xyz of the slot's box as the builder had it
    // (padded, not yet quantised).  A LEAF's box may be smaller than the bounds of its triangles: the builder splits references spatially
    // (SBVH), and a leaf then bounds only the pieces inside its cell.  The instanced scenes' refit needs these cells (instances.hip).
    bool                want_child_boxes = false;
    std::vector<float>  child_boxes;
};

// positions: [n][3][3].  Deterministic: the result does not depend on the number of builder threads (HR_BVH_THREADS, default min(hardware, 16)).
// spatial = false (deformable scenes, deform.hip): no spatial splits and no early split clipping, whatever the developer switches say — every finite
// triangle then has exactly one reference and a leaf's box is the bounds of its triangles plus the pad.
void build_bvh8(const float* positions, int n_tris, BuiltBVH& out, bool spatial = true);

// Host-side self-check (bvh_build.cpp): number of (triangle, sample point) pairs that reach no leaf holding the triangle — 0 for a
// correct tree.
int64_t check_bvh8_coverage(const float* positions, int n_tris, const BuiltBVH& b, int samples_per_triangle);

} // namespace hr
