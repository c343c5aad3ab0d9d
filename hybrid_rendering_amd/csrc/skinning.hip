// Linear-blend skinning and morph targets on MI355X (include/hr_skin.h): the stage in front of hr_scene_update_vertices / hr_scene_update_meshes
// that makes a deforming mesh's corners on the GPU.  The arithmetic of one corner is csrc/skin_math.h — the same text runs in k_skin_pose and in
// hr_skin_pose_host — and is restated in numpy by tests/skin_reference.py.
//
// k_skin_pose is a streaming kernel: one lane per corner reads 48 bytes (rest position and normal, four uint16 joints, four weights) plus 12 or
// 24 per live morph target, and writes 24.  Nothing is reused but the palette, which a workgroup stages once as 3x4 rows in LDS
// (n_joints <= kLdsJointCap) for the 256 to 2048 corners it walks, or reads through L2 above the cap; both give the same bits, they move
// the same floats.
#include "hr_internal.h"
#include "device_math.h"
#include "skin_math.h"
#include "../../include/hr_skin.h"
#include <cmath>
#include <cstring>
#include <new>

using namespace hr;

namespace hr { bool stream_is_capturing(hipStream_t st); }   // instances_shared_update.hip

namespace {

// 256 joints x 48 bytes = 12 KiB of LDS per workgroup of 4 waves: the 8 workgroups a CU holds at its 32-wave cap take 96 of its 160 KiB, so the
// staged palette never lowers the occupancy.  A workgroup walks up to 8 x 256 corners (144 KiB of stream) per palette it stages, and fewer when
// that would leave the device short of workgroups: the grid aims at SKIN_BLOCKS_PER_CU workgroups per CU (docs/EXPERIMENTS.md, "Skinning").
#ifndef SKIN_BLOCKS_PER_CU
#define SKIN_BLOCKS_PER_CU 4
#endif
constexpr int kLdsJointCap = 256, kBlock = 256, kMaxPassesPerBlock = 8;
constexpr int kMaxJoints = 65536;       // joint indices are uint16
constexpr int kMaxTris   = 1 << 28;     // 3 * n_tris corners in an int, 9 * n_tris floats addressed in 64 bits
constexpr double kMaxWeightSumError = 0.0009765625;   // 2^-10 (hr_skin_bounds)

struct SkinArgs
{
    const float*    rest_p;
    const float*    rest_n;
    const uint16_t* joints;
    const float*    weights;
    const float*    dP;
    const float*    dN;      // nullptr: normals do not morph
    const float*    J;       // [n_joints][16] column-major
    const float*    mw;      // [n_targets]; not read unless MORPH
    float*          out_p;
    float*          out_n;
    long long       n_corners;
    int             n_joints, n_targets;
    int             passes;  // 256-corner passes per workgroup, 1 .. kMaxPassesPerBlock
};

// the staged palette: joint j's row r at s[j*12 + r*4], read as one 16-byte LDS access
struct PaletteLds
{
    const float* s;
    HR_HD void row(int j, int r, float* out) const
    {
        const float4 v = *(const float4*)(s + j * 12 + r * 4);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    }
};

template <bool LDS, bool MORPH>
__global__ __launch_bounds__(kBlock) void k_skin_pose(SkinArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_pal[LDS ? kLdsJointCap * 12 : 4];
    if (LDS)
    {
        for (int e = threadIdx.x; e < a.n_joints * 12; e += kBlock)   // n_joints <= kLdsJointCap (the host picks LDS by it)
        {
            const int j = e / 12, r = (e % 12) >> 2, c = e & 3;
            s_pal[e] = a.J[j * 16 + c * 4 + r];
        }
        __syncthreads();
    }
    const long long first = (long long)blockIdx.x * (a.passes * kBlock) + threadIdx.x;
    for (int it = 0; it < a.passes; it++)
    {
        const long long i = first + it * kBlock;
        if (i >= a.n_corners) return;
        float p[3], n[3];
        for (int k = 0; k < 3; k++) { p[k] = a.rest_p[i * 3 + k]; n[k] = a.rest_n[i * 3 + k]; }
        if (MORPH)
            for (int t = 0; t < a.n_targets; t++)
            {
                const float mw = a.mw[t];   // wave-uniform
                if (mw != 0.0f)
                {
                    const long long d = ((long long)t * a.n_corners + i) * 3;
                    skin::morph3(p, mw, a.dP + d);
                    if (a.dN) skin::morph3(n, mw, a.dN + d);
                }
            }
        const uint2  jj = ((const uint2*)a.joints)[i];
        const float4 ww = ((const float4*)a.weights)[i];
        const uint16_t jn[4] = { (uint16_t)(jj.x & 0xffffu), (uint16_t)(jj.x >> 16), (uint16_t)(jj.y & 0xffffu), (uint16_t)(jj.y >> 16) };
        const float    w[4]  = { ww.x, ww.y, ww.z, ww.w };
        float M[12], op[3], on[3];
        if (LDS) skin::blend(jn, w, PaletteLds{ s_pal }, M);
        else     skin::blend(jn, w, skin::PaletteColumnMajor{ a.J }, M);
        skin::position(M, p, op);
        skin::normal(M, n, on);
        for (int k = 0; k < 3; k++) { a.out_p[i * 3 + k] = op[k]; a.out_n[i * 3 + k] = on[k]; }
    }
}

hr_status bad(const char* call, const std::string& what)
{
    set_last_error(std::string(call) + ": " + what);
    return HR_ERR_INVALID_ARG;
}

// the refusals of hr_skin_check_desc; max_err: max over the corners of |sum(w) - 1|, the four floats summed exactly (a double holds the sum)
hr_status check_desc(const char* call, const hr_skin_desc* d, double* max_err)
{
    if (!d) return bad(call, "desc is NULL");
    if (d->n_tris < 1) return bad(call, "n_tris < 1");
    if (d->n_tris > kMaxTris) { set_last_error(std::string(call) + ": more than 2^28 triangles"); return HR_ERR_UNSUPPORTED; }
    if (d->n_joints < 1) return bad(call, "n_joints < 1");
    if (d->n_joints > kMaxJoints) return bad(call, "n_joints > 65536 (joint indices are uint16)");
    if (d->n_targets < 0) return bad(call, "n_targets < 0");
    if (!d->rest_positions) return bad(call, "rest_positions is NULL");
    if (!d->rest_normals) return bad(call, "rest_normals is NULL");
    if (!d->joints) return bad(call, "joints is NULL");
    if (!d->weights) return bad(call, "weights is NULL");
    if (d->n_targets > 0 && !d->target_positions) return bad(call, "target_positions is NULL with n_targets > 0");
    const long long n = 3LL * d->n_tris;
    double worst = 0.0;
    for (long long i = 0; i < n; i++)
    {
        const float*    w = d->weights + i * 4;
        const uint16_t* j = d->joints + i * 4;
        bool   any = false;
        double sum = 0.0;
        for (int k = 0; k < 4; k++)
        {
            if (!skin::finite_f(w[k])) return bad(call, "corner " + std::to_string(i) + " slot " + std::to_string(k) + ": the weight is not finite");
            if (w[k] < 0.0f) return bad(call, "corner " + std::to_string(i) + " slot " + std::to_string(k) + ": the weight is negative");
            if (w[k] != 0.0f)
            {
                if ((int)j[k] >= d->n_joints)
                    return bad(call, "corner " + std::to_string(i) + " slot " + std::to_string(k) + ": joint index " + std::to_string((int)j[k]) + " >= n_joints with a non-zero weight");
                any = true;
            }
            sum += (double)w[k];
        }
        if (!any) return bad(call, "corner " + std::to_string(i) + ": all four weights are zero");
        worst = std::fmax(worst, std::fabs(sum - 1.0));
    }
    if (max_err) *max_err = worst;
    return HR_OK;
}

template <class F>
hr_status guarded_call(const char* call, F f)
{
    try
    {
        return f();
    }
    catch (const std::bad_alloc&)
    {
        set_last_error(std::string(call) + ": host allocation failed");
        return HR_ERR_OUT_OF_MEMORY;
    }
    catch (const std::exception& e)
    {
        set_last_error(std::string(call) + ": " + e.what());
        return HR_ERR_UNSUPPORTED;
    }
}

} // namespace

struct hr_skin
{
    hr_ctx* ctx = nullptr;
    int     n_tris = 0, n_joints = 0, n_targets = 0;
    bool    has_dn = false;
    double  max_weight_sum_error = 0.0;
    DevBuf  rest_p, rest_n, joints, weights, dP, dN, out_p, out_n;
    DevBuf  pal_dev, mw_dev;                 // where hr_skin_pose stages the host palette and morph weights for the kernel
    float*  stage = nullptr;                 // pinned: [n_joints][16] then [n_targets]
    hipEvent_t staged = nullptr;             // recorded behind the copies out of `stage`
    bool    staged_pending = false;
    // hr_skin_bounds: per joint, whether a corner uses it with a non-zero weight, the rest box of those corners, and per target the largest
    // |dP| of those corners per axis
    std::vector<uint8_t> joint_used;
    std::vector<float>   joint_lo, joint_hi, joint_dmax;
    StageProfiler prof;
    ~hr_skin()
    {
        if (staged) (void)hipEventDestroy(staged);
        if (stage) (void)hipHostFree(stage);
    }
};

namespace {

hr_status create_impl(hr_ctx* ctx, const hr_skin_desc* d, hr_skin** out)
{
    static const char* call = "hr_skin_create";
    if (out) *out = nullptr;
    double werr = 0.0;
    hr_status e = check_desc(call, d, &werr);
    if (e != HR_OK) return e;
    if (!out) return bad(call, "out is NULL");
    if (ctx) HR_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<hr_skin> s(new hr_skin());
    s->ctx = ctx; s->n_tris = d->n_tris; s->n_joints = d->n_joints; s->n_targets = d->n_targets;
    s->has_dn = d->n_targets > 0 && d->target_normals != nullptr;
    s->max_weight_sum_error = werr;
    const size_t nc = (size_t)3 * d->n_tris, nt = (size_t)d->n_targets;

    // the bound's tables
    const float inf = INFINITY;
    s->joint_used.assign(d->n_joints, 0);
    s->joint_lo.assign((size_t)d->n_joints * 3, inf);
    s->joint_hi.assign((size_t)d->n_joints * 3, -inf);
    s->joint_dmax.assign((size_t)d->n_joints * nt * 3, 0.0f);
    for (size_t i = 0; i < nc; i++)
        for (int k = 0; k < 4; k++)
        {
            if (d->weights[i * 4 + k] == 0.0f) continue;
            const size_t j = d->joints[i * 4 + k];
            s->joint_used[j] = 1;
            for (int c = 0; c < 3; c++)
            {
                const float v = d->rest_positions[i * 3 + c];
                s->joint_lo[j * 3 + c] = imath::fmin_(s->joint_lo[j * 3 + c], v);
                s->joint_hi[j * 3 + c] = imath::fmax_(s->joint_hi[j * 3 + c], v);
                for (size_t t = 0; t < nt; t++)
                {
                    float& m = s->joint_dmax[(j * nt + t) * 3 + c];
                    m = imath::fmax_(m, std::fabs(d->target_positions[(t * nc + i) * 3 + c]));
                }
            }
        }

    if (!ctx)   // a host-only skin: hr_skin_info and hr_skin_bounds
    {
        *out = s.release();
        return HR_OK;
    }
    struct Up { DevBuf* b; const void* src; size_t bytes; };
    const Up ups[] = { { &s->rest_p, d->rest_positions, nc * 12 }, { &s->rest_n, d->rest_normals, nc * 12 }, { &s->joints, d->joints, nc * 8 },
                       { &s->weights, d->weights, nc * 16 }, { &s->dP, d->target_positions, nt * nc * 12 }, { &s->dN, s->has_dn ? d->target_normals : nullptr, nt * nc * 12 },
                       { &s->out_p, d->rest_positions, nc * 12 }, { &s->out_n, d->rest_normals, nc * 12 } };
    for (const Up& u : ups)
    {
        if (!u.src || u.bytes == 0) continue;
        if ((e = u.b->alloc(u.bytes)) != HR_OK) return e;
        HR_HIP(hipMemcpy(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice));
    }
    if ((e = s->pal_dev.alloc((size_t)d->n_joints * 64)) != HR_OK) return e;
    if ((e = s->mw_dev.alloc(nt * 4)) != HR_OK) return e;
    HR_HIP(hipHostMalloc((void**)&s->stage, ((size_t)d->n_joints * 16 + nt + 1) * 4, hipHostMallocDefault));
    HR_HIP(hipEventCreateWithFlags(&s->staged, hipEventDisableTiming));
    *out = s.release();
    return HR_OK;
}

bool finite_n(const float* v, size_t n)
{
    bool ok = true;
    for (size_t i = 0; i < n; i++) ok = ok && skin::finite_f(v[i]);
    return ok;
}

// what hr_skin_pose and hr_skin_bounds refuse: a used joint's matrix or a morph weight that is not finite
hr_status check_pose(const char* call, const hr_skin* s, const float* matrices, const float* mw)
{
    if (!s) return bad(call, "skin is NULL");
    if (!matrices) return bad(call, "joint_matrices_host is NULL");
    for (int j = 0; j < s->n_joints; j++)
        if (s->joint_used[j] && !imath::finite16(matrices + (size_t)j * 16)) return bad(call, "the matrix of joint " + std::to_string(j) + " is not finite");
    if (mw && !finite_n(mw, (size_t)s->n_targets)) return bad(call, "a morph weight is not finite");
    return HR_OK;
}

} // namespace

extern "C" {

hr_status hr_skin_check_desc(const hr_skin_desc* desc)
{
    return guarded_call("hr_skin_check_desc", [&] { return check_desc("hr_skin_check_desc", desc, nullptr); });
}

hr_status hr_skin_create(hr_ctx* ctx, const hr_skin_desc* desc, hr_skin** out)
{
    return guarded_call("hr_skin_create", [&] { return create_impl(ctx, desc, out); });
}

hr_status hr_skin_destroy(hr_skin* skin)
{
    if (!skin) return HR_OK;
    if (skin->ctx) (void)hipSetDevice(skin->ctx->device);
    if (skin->staged_pending) (void)hipEventSynchronize(skin->staged);
    delete skin;
    return HR_OK;
}

hr_status hr_skin_info(const hr_skin* skin, hr_skin_info_data* out)
{
    if (!skin) return bad("hr_skin_info", "skin is NULL");
    if (!out) return bad("hr_skin_info", "out is NULL");
    out->n_tris = skin->n_tris; out->n_joints = skin->n_joints; out->n_targets = skin->n_targets;
    out->lds_joint_cap = kLdsJointCap;
    // rounded up: the value reported is never below the one hr_skin_bounds compares
    float f = (float)skin->max_weight_sum_error;
    if ((double)f < skin->max_weight_sum_error) f = imath::next_up(f);
    out->max_weight_sum_error = f;
    return HR_OK;
}

hr_status hr_skin_output(const hr_skin* skin, const float** positions, const float** normals)
{
    if (!skin) return bad("hr_skin_output", "skin is NULL");
    if (!skin->ctx) return bad("hr_skin_output", "a host-only skin (created with ctx NULL) has no device buffers");
    if (positions) *positions = (const float*)skin->out_p.p;
    if (normals) *normals = (const float*)skin->out_n.p;
    return HR_OK;
}

hr_status hr_skin_pose_device(hr_skin* s, const float* joint_matrices_device, const float* morph_weights_device, void* stream)
{
    static const char* call = "hr_skin_pose_device";
    if (!s) return bad(call, "skin is NULL");
    if (!joint_matrices_device) return bad(call, "joint_matrices_device is NULL");
    if (!s->ctx) return bad(call, "a host-only skin (created with ctx NULL) cannot pose");
    HR_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const bool morph = morph_weights_device != nullptr && s->n_targets > 0, lds = s->n_joints <= kLdsJointCap;
    SkinArgs a;
    a.rest_p = (const float*)s->rest_p.p; a.rest_n = (const float*)s->rest_n.p;
    a.joints = (const uint16_t*)s->joints.p; a.weights = (const float*)s->weights.p;
    a.dP = (const float*)s->dP.p; a.dN = s->has_dn ? (const float*)s->dN.p : nullptr;
    a.J = joint_matrices_device; a.mw = morph_weights_device;
    a.out_p = (float*)s->out_p.p; a.out_n = (float*)s->out_n.p;
    a.n_corners = 3LL * s->n_tris; a.n_joints = s->n_joints; a.n_targets = s->n_targets;
    const long long cus = s->ctx->props.multiProcessorCount > 0 ? s->ctx->props.multiProcessorCount : 256;
    const long long fit = a.n_corners / (kBlock * cus * SKIN_BLOCKS_PER_CU);
    a.passes = (int)(fit < 1 ? 1 : (fit > kMaxPassesPerBlock ? kMaxPassesPerBlock : fit));
    const long long per_block = (long long)a.passes * kBlock;
    const unsigned blocks = (unsigned)((a.n_corners + per_block - 1) / per_block);
    const uint64_t bytes = (uint64_t)a.n_corners * (48 + 24 + (morph ? (uint64_t)s->n_targets * (s->has_dn ? 24 : 12) : 0)) + (uint64_t)s->n_joints * 48;
    s->prof.begin_frame();
    const int ev = s->prof.begin("skin_pose", st, bytes);
    if (lds && morph)       hipLaunchKernelGGL((k_skin_pose<true, true>), dim3(blocks), dim3(kBlock), 0, st, a);
    else if (lds)           hipLaunchKernelGGL((k_skin_pose<true, false>), dim3(blocks), dim3(kBlock), 0, st, a);
    else if (morph)         hipLaunchKernelGGL((k_skin_pose<false, true>), dim3(blocks), dim3(kBlock), 0, st, a);
    else                    hipLaunchKernelGGL((k_skin_pose<false, false>), dim3(blocks), dim3(kBlock), 0, st, a);
    s->prof.end(ev, st);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_skin_pose(hr_skin* s, const float* joint_matrices_host, const float* morph_weights_host, void* stream)
{
    static const char* call = "hr_skin_pose";
    const hr_status c = check_pose(call, s, joint_matrices_host, morph_weights_host);
    if (c != HR_OK) return c;
    if (!s->ctx) return bad(call, "a host-only skin (created with ctx NULL) cannot pose");
    HR_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st)) return bad(call, "the stream is capturing: the staging copy cannot be replayed (capture hr_skin_pose_device)");
    // the previous call's copies out of `stage` have run before it is written again (its kernels may still be running: they read pal_dev / mw_dev,
    // and this call's copies are ordered behind them on the stream)
    if (s->staged_pending) { HR_HIP(hipEventSynchronize(s->staged)); s->staged_pending = false; }
    const size_t nj = (size_t)s->n_joints * 16;
    const bool   morph = morph_weights_host != nullptr && s->n_targets > 0;
    std::memcpy(s->stage, joint_matrices_host, nj * 4);
    if (morph) std::memcpy(s->stage + nj, morph_weights_host, (size_t)s->n_targets * 4);
    HR_HIP(hipMemcpyAsync(s->pal_dev.p, s->stage, nj * 4, hipMemcpyHostToDevice, st));
    if (morph) HR_HIP(hipMemcpyAsync(s->mw_dev.p, s->stage + nj, (size_t)s->n_targets * 4, hipMemcpyHostToDevice, st));
    HR_HIP(hipEventRecord(s->staged, st));
    s->staged_pending = true;
    return hr_skin_pose_device(s, (const float*)s->pal_dev.p, morph ? (const float*)s->mw_dev.p : nullptr, stream);
}

// The box.  Write p^ for a corner's morphed position as the kernel computes it, y_k = J_k p^ (exact) for its live slots, s = sum(w_k).
//  (1) Morph: p^ is a chain of 2 roundings per live target over terms bounded by |rest| + sum_t |mw_t| |dP_t|, so per axis it lies within
//      D = sum_t |mw_t| max|dP_t| of the joint's rest box, plus ((1 + u)^(2 n) - 1) * A <= 2 n * 2^-23 * A, with u = 2^-24, n the live targets
//      and A the largest magnitude of the box widened by D.  The widened box B_j therefore holds p^ for every corner joint j influences.
//  (2) Blend and position: every product w_k * J_k[r][c] * p^_c reaches out_p[r] through at most 8 roundings (the product T, up to 3 sums into
//      M, the product with p^_c, up to 3 sums of the row), so |out_p[r] - sum_k w_k y_k[r]| <= ((1 + u)^8 - 1) * sum_k w_k e_k[r], where
//      e_k[r] = sum_c |J_k[r][c]| |p^_c| + |J_k[r][3]| <= E[r], the largest such sum over the corners of the boxes B_j.  2^-20 = 16 u is twice
//      the first-order term: it covers the higher orders and the double-precision evaluation below.
//  (3) Weights: sum_k w_k y_k = s * ybar with ybar a convex combination (w_k >= 0) of points of the images J_j(B_j), so inside their union U,
//      and |s * ybar - ybar| <= |s - 1| * E[r].
//  Hence out_p[r] lies within  pad[r] = (|s - 1|_max + 2^-20 * (1 + |s - 1|_max)) * E[r]  of U; 2^-140 on top covers products that
//  underflow (an absolute 2^-150 each), and lo / hi are rounded outwards to float.
hr_status hr_skin_bounds(const hr_skin* s, const float* joint_matrices_host, const float* morph_weights_host, float out[6])
{
    static const char* call = "hr_skin_bounds";
    const hr_status c = check_pose(call, s, joint_matrices_host, morph_weights_host);
    if (c != HR_OK) return c;
    if (!out) return bad(call, "out is NULL");
    if (s->max_weight_sum_error > kMaxWeightSumError)
    {
        set_last_error(std::string(call) + ": the skin's weights sum to 1 only within " + std::to_string(s->max_weight_sum_error) + " (> 2^-10): no rounding-level box exists; pass bounds = NULL");
        return HR_ERR_UNSUPPORTED;
    }
    const int    nt   = morph_weights_host ? s->n_targets : 0;
    int          live = 0;
    for (int t = 0; t < nt; t++) live += morph_weights_host[t] != 0.0f ? 1 : 0;
    double L[3] = { 1e300, 1e300, 1e300 }, H[3] = { -1e300, -1e300, -1e300 }, E[3] = { 0.0, 0.0, 0.0 };
    for (int j = 0; j < s->n_joints; j++)
    {
        if (!s->joint_used[j]) continue;
        const float* m = joint_matrices_host + (size_t)j * 16;
        double lo[3], hi[3];
        for (int a = 0; a < 3; a++)
        {
            lo[a] = (double)s->joint_lo[(size_t)j * 3 + a]; hi[a] = (double)s->joint_hi[(size_t)j * 3 + a];
            double D = 0.0;
            for (int t = 0; t < nt; t++) D += std::fabs((double)morph_weights_host[t]) * (double)s->joint_dmax[((size_t)j * s->n_targets + t) * 3 + a];
            const double A = std::fmax(std::fabs(lo[a]), std::fabs(hi[a])) + D;
            D += 2.0 * live * 1.1920928955078125e-7 * A;   // (1)
            lo[a] -= D; hi[a] += D;
        }
        for (int q = 0; q < 8; q++)
        {
            const double x = (q & 1) ? hi[0] : lo[0], y = (q & 2) ? hi[1] : lo[1], z = (q & 4) ? hi[2] : lo[2];
            for (int r = 0; r < 3; r++)
            {
                const double tx = (double)m[r] * x, ty = (double)m[4 + r] * y, tz = (double)m[8 + r] * z, tw = (double)m[12 + r];
                const double v = tx + ty + tz + tw, e = std::fabs(tx) + std::fabs(ty) + std::fabs(tz) + std::fabs(tw);
                L[r] = imath::dmin(L[r], v); H[r] = imath::dmax(H[r], v); E[r] = imath::dmax(E[r], e);
            }
        }
    }
    const double ws = s->max_weight_sum_error;
    for (int r = 0; r < 3; r++)
    {
        const double pad = (ws + 9.5367431640625e-7 * (1.0 + ws)) * E[r] + 7.174648137343064e-43;   // (2), (3); 2^-20, 2^-140
        const double l = L[r] - pad, h = H[r] + pad;
        float lf = (float)l, hf = (float)h;
        if ((double)lf > l) lf = imath::next_down(lf);
        if ((double)hf < h) hf = imath::next_up(hf);
        out[r] = lf; out[3 + r] = hf;
    }
    return HR_OK;
}

hr_status hr_skin_pose_host(const hr_skin_desc* d, const float* matrices, const float* morph_weights, float* out_positions, float* out_normals)
{
    static const char* call = "hr_skin_pose_host";
    return guarded_call(call, [&]() -> hr_status {
        const hr_status c = check_desc(call, d, nullptr);
        if (c != HR_OK) return c;
        if (!matrices) return bad(call, "matrices is NULL");
        if (!out_positions) return bad(call, "out_positions is NULL");
        const long long nc = 3LL * d->n_tris;
        const int       nt = morph_weights ? d->n_targets : 0;
        const skin::PaletteColumnMajor pal = { matrices };
        for (long long i = 0; i < nc; i++)
        {
            float p[3], n[3], M[12];
            for (int k = 0; k < 3; k++) { p[k] = d->rest_positions[i * 3 + k]; n[k] = d->rest_normals[i * 3 + k]; }
            for (int t = 0; t < nt; t++)
            {
                const float mw = morph_weights[t];
                if (mw != 0.0f)
                {
                    const long long o = ((long long)t * nc + i) * 3;
                    skin::morph3(p, mw, d->target_positions + o);
                    if (d->target_normals) skin::morph3(n, mw, d->target_normals + o);
                }
            }
            skin::blend(d->joints + i * 4, d->weights + i * 4, pal, M);
            skin::position(M, p, out_positions + i * 3);
            if (out_normals) skin::normal(M, n, out_normals + i * 3);
        }
        return HR_OK;
    });
}

hr_status hr_skin_set_profiling(hr_skin* skin, int32_t enable)
{
    if (!skin) return bad("hr_skin_set_profiling", "skin is NULL");
    skin->prof.enabled = enable != 0;
    return HR_OK;
}

hr_status hr_skin_get_stage_times(hr_skin* skin, hr_stage_times* out)
{
    if (!skin) return bad("hr_skin_get_stage_times", "skin is NULL");
    if (!out) return bad("hr_skin_get_stage_times", "out is NULL");
    if (skin->ctx) HR_HIP(hipSetDevice(skin->ctx->device));
    skin->prof.collect(out);
    return HR_OK;
}

} // extern "C"
