// The refit of split-free trees under new vertices (deform_refit.hip): the one engine of the flat deformable scenes (deform.hip: one mesh, root 0)
// and of the deforming meshes of a shared instanced scene (instances_shared_deform.hip).  Its state is the scene's DeformRefit (hr_internal.h).
#pragma once
#include "hr_internal.h"

namespace hr {

constexpr int kMaxUpdatesPerLaunch = 64;    // scatter entries, and so meshes, one set of launches takes: the tables travel as kernel arguments

// one mesh of deform_refit_adopt
struct DeformMesh
{
    const BuiltBVH* bvh;            // built without spatial splits when `flag`
    uint32_t        root;           // node index of its root in the scene's `nodes`
    uint32_t        ref_base;       // its first reference in the scene's `tris`
    uint32_t        tri_base;       // its first triangle in the attribute arrays the scatter writes
    int32_t         n_tris;
    float           pad;            // the leaf pad its builder used (not read: a refit derives the pad from the mesh's current bounds)
    bool            flag;           // may be updated
    int             narrow;         // levels of at most this many nodes, from the root down to the first wider one, stay in the mesh's own workgroup
};

// `s` holds the uploaded trees and info.n_nodes: level lists, triangle -> reference map and partial slots of every flagged mesh, node_box (by one
// refit into a scratch copy of the nodes: the scene's own stay as built) and the cost of every flagged tree as built.  Replaces s->deform and
// s->node_box only when all of it has succeeded: after a failure the scene refits as before.  Synchronous, like creation.  `call` heads the
// error messages.
hr_status deform_refit_adopt(hr_scene* s, const std::vector<DeformMesh>& meshes, const char* call);

// new vertices of triangles [first, first + count) of a flagged mesh, device memory; normals may be null
struct DeformScatterEntry { const float* positions; const float* normals; uint32_t mesh; int32_t first, count; };
// one launch for all n <= kMaxUpdatesPerLaunch entries: the references' vertex bytes and the entries' rows of dst_positions / dst_normals
void deform_refit_scatter(hr_scene* s, const DeformScatterEntry* e, int n, float* dst_positions, float* dst_normals, hipStream_t st);

// the refit of the flagged meshes ms[0 .. n) (at most kMaxUpdatesPerLaunch, distinct) into `nodes`; bounds: null, or per entry of `ms` the caller's
// bounds of that mesh (6 floats) or null
hr_status deform_refit_enqueue(hr_scene* s, Node8* nodes, const uint32_t* ms, int n, const float* const* bounds, hipStream_t st);

// the first launch of deform_refit_enqueue alone: the exact bounds of the finite references of ms[0 .. n) into their words of bounds_bits, which
// must stand idle.  Whoever calls it puts the words back before the next refit (deform_redeal.hip: its commit launch)
void deform_refit_bounds_enqueue(hr_scene* s, const uint32_t* ms, int n, hipStream_t st);

// Depth-first list of a tree's reference slots (slots of a node in slot order, a leaf's triangles in offset order), relative to the tree's first
// reference.  `nodes`: n_nodes nodes whose child_base index that array, `root` among them.  false: a child outside the array, more than
// `capacity` references, or more node visits than nodes (not a tree); nothing is written then.
bool deform_leaf_order(const Node8* nodes, int32_t n_nodes, uint32_t root, int32_t* slot_of_rank, int32_t capacity, int32_t* n);

// deform_redeal.hip: the triangles of the flagged meshes ms[0 .. n) (at most kMaxUpdatesPerLaunch, distinct) re-dealt among their standing reference
// slots in Morton order, then deform_refit_enqueue over all of them (bounds as there).  Kernels only on `st`; allocates at a scene's first call.
hr_status deform_redeal_enqueue(hr_scene* s, const uint32_t* ms, int n, hipStream_t st);

// sum of mesh m's half areas now / when built; reads the slots back when an update ran since the last call (cost_known[m] == 0): the caller has
// synchronised the device by then
hr_status deform_refit_cost(hr_scene* s, uint32_t m, float* ratio);

} // namespace hr
