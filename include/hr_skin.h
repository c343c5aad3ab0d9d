/* hr_skin.h — linear-blend skinning and morph targets on the GPU: what produces, every frame, the triangle corners that
 * hr_scene_update_vertices and hr_scene_update_meshes take from device memory, C ABI.  (The reference has no counterpart: it loads static
 * meshes and rebuilds its top level per frame, main.cpp:74.  The contract below is the specification; tests/skin_reference.py restates it in
 * numpy.)
 *
 * A skin is a triangle stream in the project's own unindexed layout — [n_tris][3][3] rest positions and normals, corner i = 3*triangle +
 * vertex — with four (joint, weight) influences per corner and n_targets morph targets of per-corner deltas.  hr_skin_create uploads it once
 * and owns two device output buffers of the same layout; hr_skin_pose_device / hr_skin_pose fill them for one pose on the caller's stream.
 * Calls on one hr_skin are externally serialised.
 *
 * Library: hybrid_rendering_amd/libhybrid_rendering_amd.so (csrc/skinning.hip; the per-corner function is csrc/skin_math.h, one text for the
 * kernel and for hr_skin_pose_host).
 *
 * ---- Contract: every fp32 operation is one correctly rounded operation, nothing is contracted, sums are taken in the order written ------
 * Per corner i, with J = the caller's palette [n_joints][16], column-major 4x4 as everywhere in this API (J[j][r][c] = m[c*4 + r]; the last
 * row is not read), mw = the morph weights [n_targets]:
 *   Morph.     p = rest_p[i];  for t = 0 .. n_targets-1 in order, when mw[t] != 0:  p = p + mw[t]*dP[t][i]  (the product is rounded, then the
 *              sum).  The normal n = rest_n[i] takes dN[t][i] the same way when the skin has normal deltas.  A target with mw[t] == 0 is
 *              skipped (a select, not a multiply).  No morph weights given: no target applies.
 *   Blend.     For slots k = 0..3 in order, slot k contributes iff w[i][k] != 0 (+0 and -0 do not).  For r = 0..2, c = 0..3:
 *              T = w[i][k] * J[joint[i][k]][r][c];  M[r][c] = T for the first contributing slot, M[r][c] + T afterwards.
 *              Skipping is part of the contract: a slot of weight zero is not read, so it may name a joint whose matrix is not finite (or no
 *              joint of the skin at all), and 0 * inf never reaches a vertex.
 *   Position.  out_p[r] = ((M[r][0]*p.x + M[r][1]*p.y) + M[r][2]*p.z) + M[r][3].
 *   Normal.    v[r] = (M[r][0]*n.x + M[r][1]*n.y) + M[r][2]*n.z  — mat3 of the blended matrix, as the instance transform of this API does, not
 *              the inverse transpose;  l2 = (v0*v0 + v1*v1) + v2*v2;  when l2 > 0 and finite: out_n[r] = v[r] / sqrt(l2) (an IEEE square root,
 *              three IEEE divisions); otherwise out_n = v as it stands (a zero, infinite or NaN normal is stored, not repaired).
 *
 * ---- Out of scope ----------------------------------------------------------------------------------------------------------------------
 *   * Tangents are not re-posed: hr_scene_update_vertices has no tangent input, so a normal-mapped skinned mesh keeps its rest tangents.
 *   * Dual-quaternion skinning.
 *   * More than four influences per corner (glTF JOINTS_1 / WEIGHTS_1).
 *   * Animation sampling: integrators bring their own palettes (the Python package samples glTF animations: assets.load_gltf_skinned).
 *   * An indexed variant (skin each vertex once, then expand by index): not built and not costed; every corner is skinned.
 */
#ifndef HR_SKIN_H
#define HR_SKIN_H

#include "hr_api.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hr_skin hr_skin;

typedef struct
{
    int32_t         n_tris;           /* >= 1 */
    int32_t         n_joints;         /* 1 .. 65536 */
    const float*    rest_positions;   /* HOST [n_tris][3][3] */
    const float*    rest_normals;     /* HOST [n_tris][3][3] */
    const uint16_t* joints;           /* HOST [n_tris][3][4] */
    const float*    weights;          /* HOST [n_tris][3][4]: finite, >= 0, not all four zero; their sum SHOULD be 1 (hr_skin_bounds) */
    int32_t         n_targets;        /* >= 0 */
    const float*    target_positions; /* HOST [n_targets][n_tris][3][3] position deltas; may be NULL when n_targets == 0 */
    const float*    target_normals;   /* HOST [n_targets][n_tris][3][3] normal deltas, or NULL: normals do not morph */
} hr_skin_desc;                       /* 64 bytes */

typedef struct
{
    int32_t n_tris, n_joints, n_targets;
    int32_t lds_joint_cap;       /* the kernel stages the palette in LDS when n_joints <= this, and reads it through L2 above; same bits */
    float   max_weight_sum_error; /* max over the corners of |sum(w) - 1| (the four floats summed exactly) */
} hr_skin_info_data;

/* Host only, no device is needed.  HR_ERR_INVALID_ARG, naming the cause in hr_last_error(): desc or a required array NULL, n_tris < 1,
 * n_joints < 1 or > 65536, n_targets < 0, a joint index >= n_joints in a slot whose weight is not zero, a weight that is negative or not
 * finite, a corner whose four weights are all zero.  Never throws. */
hr_status hr_skin_check_desc(const hr_skin_desc* desc);
/* hr_skin_check_desc first, before anything is allocated; then uploads the arrays (synchronous) and allocates the outputs, which start as
 * the rest pose's positions and normals.  ctx == NULL: a host-only skin, which needs no device and serves hr_skin_info and hr_skin_bounds;
 * posing it or asking for its outputs is HR_ERR_INVALID_ARG. */
hr_status hr_skin_create(hr_ctx* ctx, const hr_skin_desc* desc, hr_skin** out);
hr_status hr_skin_destroy(hr_skin* skin);
hr_status hr_skin_info(const hr_skin* skin, hr_skin_info_data* out);

/* joint_matrices_device: DEVICE [n_joints][16];  morph_weights_device: DEVICE [n_targets] or NULL (no target applies, and the launch does
 * not pay for the morph loop).  Launches kernels only: no allocation, no host wait, legal under stream capture — both arrays are read when
 * the launch runs, so a replay poses from what they then hold. */
hr_status hr_skin_pose_device(hr_skin* skin, const float* joint_matrices_device, const float* morph_weights_device, void* stream);
/* The same from HOST arrays: the matrices of every joint that some corner uses with a non-zero weight, and the morph weights, must be finite
 * (HR_ERR_INVALID_ARG before anything is enqueued; a joint no corner uses is never read by the kernel and is not checked).  Staged through a
 * pinned buffer the skin owns, which the call does not overwrite before the previous call's copy out of it has run (it waits for that copy,
 * not for the kernels).  Not under stream capture (HR_ERR_INVALID_ARG): capture hr_skin_pose_device. */
hr_status hr_skin_pose(hr_skin* skin, const float* joint_matrices_host, const float* morph_weights_host, void* stream);
/* DEVICE [n_tris][3][3] each, stable for the skin's life: what hr_scene_update_vertices(scene, positions, normals, first_tri, n_tris, stream)
 * takes as they are (a skin may cover a sub-range of a flat deformable scene), and hr_mesh_update.positions / .normals likewise. */
hr_status hr_skin_output(const hr_skin* skin, const float** positions, const float** normals);

/* Host only, once the skin exists: a conservative object-space box (lo xyz, hi xyz) of every position the kernel writes for this pose —
 * what hr_mesh_update.bounds asks for, so that a shared scene updates without its stream wait.  Per joint, the rest box of the corners it
 * influences, widened by sum_t |mw[t]| * max |dP[t]| over those corners, goes through that joint's matrix in double; the union is padded for
 * the fp32 error of the contract's operations and for |sum(w) - 1| (the derivation stands next to the code).  HR_ERR_INVALID_ARG: a used
 * joint's matrix or a morph weight is not finite.  HR_ERR_UNSUPPORTED: the skin's max_weight_sum_error exceeds 2^-10 — the box would not be
 * a rounding-level statement any more; pass bounds = NULL to the update then. */
hr_status hr_skin_bounds(const hr_skin* skin, const float* joint_matrices_host, const float* morph_weights_host, float out[6]);

/* Host only, no device is needed: the contract in a loop over the corners (csrc/skin_math.h), for tests and integrators.  hr_skin_check_desc
 * first.  matrices: [n_joints][16];  morph_weights: [n_targets] or NULL;  out_positions: [n_tris][3][3];  out_normals: likewise, or NULL. */
hr_status hr_skin_pose_host(const hr_skin_desc* desc, const float* matrices, const float* morph_weights, float* out_positions, float* out_normals);

/* Stage skin_pose.  Profiling must be off while a pose is captured: timing events cannot be read back from a captured launch. */
hr_status hr_skin_set_profiling(hr_skin* skin, int32_t enable);
hr_status hr_skin_get_stage_times(hr_skin* skin, hr_stage_times* out);

#ifdef __cplusplus
}
#endif
#endif
