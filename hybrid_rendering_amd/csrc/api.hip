// C-ABI glue: context, scene (BVH build + upload), raw ray queries, G-buffer synthesis (one kernel body for flat and shared instanced scenes).
#include "hr_internal.h"
#include "scene_create.h"
#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include "traverse.h"
#include "traverse2.h"
#include "shading.h"
#include "pixel_dir.h"
#include "cutout_host.h"
#include "selftest.h"
#include <cstring>
#include <cmath>

using namespace hr;

namespace hr {
static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
} // namespace hr

// ------------------------------------------------------------------------------------------------
// profiler ranges (hr_internal.h): roctx through dlopen — the library is only needed when somebody asks for markers
#include <dlfcn.h>
#include <cstdlib>
#include <mutex>
namespace hr {
namespace {
std::atomic<int> g_marker_mode { -1 };   // -1: not decided (HR_MARKERS), 0 off, 1 roctx, 2 in-process log
int  (*g_roctx_push)(const char*) = nullptr;
int  (*g_roctx_pop)() = nullptr;
std::mutex               g_marker_mutex;
std::vector<std::string> g_marker_log;   // mode 2: "+name" / "-" in call order, capped
int marker_mode()
{
    int m = g_marker_mode.load(std::memory_order_relaxed);
    if (m >= 0) return m;
    const char* e = getenv("HR_MARKERS");
    m = e ? atoi(e) : 0;
    if (m < 0 || m > 2) m = 0;
    g_marker_mode.store(m);
    return m;
}
bool roctx_ready()
{
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* lib : { "librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4" })
            if (void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL))
            {
                g_roctx_push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                g_roctx_pop  = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (g_roctx_push && g_roctx_pop) return;
            }
        g_roctx_push = nullptr; g_roctx_pop = nullptr;
    });
    return g_roctx_push && g_roctx_pop;
}
} // namespace
bool samples_on() { return marker_mode() != 0; }
void sample_push(const char* name)
{
    const int m = marker_mode();
    if (m == 1) { if (roctx_ready()) (void)g_roctx_push(name); }
    else if (m == 2) { std::lock_guard<std::mutex> l(g_marker_mutex); if (g_marker_log.size() < 4096) g_marker_log.push_back(std::string("+") + name); }
}
void sample_pop()
{
    const int m = marker_mode();
    if (m == 1) { if (roctx_ready()) (void)g_roctx_pop(); }
    else if (m == 2) { std::lock_guard<std::mutex> l(g_marker_mutex); if (g_marker_log.size() < 4096) g_marker_log.push_back("-"); }
}
const char* sample_name_of_stage(const char* stage)
{
    static const struct { const char* stage; const char* label; } table[] = {
        { "ray_trace", "Ray Trace" }, { "temporal_accumulation", "Temporal Accumulation" }, { "upsample", "Upsample" },
        { "atrous_0", "Iteration 0" }, { "atrous_1", "Iteration 1" }, { "atrous_2", "Iteration 2" }, { "atrous_3", "Iteration 3" }, { "atrous_4", "Iteration 4" },
        { "atrous_01", "Iteration 0 + Iteration 1" },   // the tolerance mode runs the first two iterations in one launch
        { "blur_x", "Vertical" }, { "blur_y", "Horizontal" },   // the reference's labels: its "Vertical" pass blurs along (1, 0) (ray_traced_ao.cpp:1042,1066)
        { "blur_xy", "Vertical + Horizontal" },
        { "probe_update", "Irradiance + Depth + Border Update" },   // one launch for the three (ddgi.hip k_ddgi_probe_update)
        { "sample_probe_grid", "Sample Probe Grid" },
        { "path_trace", "Ground Truth Path Trace" }, { "taa", "TAA" },
        { "env_sh9", "Cubemap SH Projection" }, { "env_prefilter", "Cubemap Prefilter" }, { "env_brdf_lut", "BRDF Integrate LUT" },   // the framework's passes behind hr_env (env.hip)
        { "env_equirect", "Equirectangular To Cubemap" }, { "env_sky", "Sky Model" },   // what fills the env's sky (env_sources.hip)
        { "skin_pose", "Skinning" },   // hr_skin.h (skinning.hip); the reference has static meshes only
    };
    for (const auto& t : table)
        if (std::strcmp(t.stage, stage) == 0) return t.label;
    return stage;
}
} // namespace hr

extern "C" hr_status hr_set_markers(int32_t mode)
{
    HR_CHECK_ARG(mode >= 0 && mode <= 2);
    hr::g_marker_mode.store(mode);
    std::lock_guard<std::mutex> l(hr::g_marker_mutex);
    hr::g_marker_log.clear();
    return HR_OK;
}
extern "C" int32_t hr_markers_log(char* out, int32_t capacity)
{
    std::lock_guard<std::mutex> l(hr::g_marker_mutex);
    std::string s;
    for (const std::string& e : hr::g_marker_log) { s += e; s += '\n'; }
    if (out && capacity > 0)
    {
        const size_t n = std::min(s.size(), (size_t)capacity - 1);
        std::memcpy(out, s.data(), n);
        out[n] = 0;
    }
    return (int32_t)s.size();
}

// ------------------------------------------------------------------------------------------------
// raw ray queries.  CUTOUT (all four kernels): the walks run the alpha test (cutout.h) through `cv`; the host picks it iff cutout_on(scene, HR_RAY_QUERY)
template <bool CUTOUT>
__global__ __launch_bounds__(256) void k_any_hit_batch(const Node8* nodes, const TriGPU* tris, long long n, const float* rays, uint8_t* out, unsigned long long* stats, CutoutView cv)
{
    __shared__ uint32_t s_stack[4][HR_STACK_ENTRIES * 64];
    __shared__ CoopWave s_coop[4];
    const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i    = (long long)blockIdx.x * 256 + threadIdx.x;
    uint32_t        nn = 0, nt = 0;
    // the counting query walks per lane (trace_any); the plain one is the wave-cooperative walk the AO pass uses (trace_coop)
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (i < n) { a = ((const float4*)rays)[i * 2]; b = ((const float4*)rays)[i * 2 + 1]; }
    if (!CUTOUT && stats)
    {
        if (i < n) out[i] = trace_any<true>(nodes, tris, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), b.w, a.w, s_stack[wave], lane, nn, nt) ? 1 : 0;
    }
    else
    {
        const bool occ = trace_coop<true, HR_ANY_ORDER, CUTOUT>(i < n, nodes, tris, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), b.w, a.w, s_stack[wave], s_coop[wave], lane, 0u, nullptr, cv).prim == 0;
        if (i < n) out[i] = occ ? 1 : 0;
    }
    if (!CUTOUT && stats)
    {
        for (int o = 32; o > 0; o >>= 1) { nn += __shfl_down(nn, o); nt += __shfl_down(nt, o); }
        if (lane == 0)
        {
            atomicAdd(stats + 0, (unsigned long long)nn);
            atomicAdd(stats + 1, (unsigned long long)nt);
        }
    }
}

template <bool CUTOUT>
__global__ __launch_bounds__(256) void k_closest_hit_batch(const Node8* nodes, const TriGPU* tris, long long n, const float* rays, float* out_tuv, int32_t* out_prim, CutoutView cv)
{
    __shared__ uint32_t s_stack[4][HR_STACK_ENTRIES * 64];
    __shared__ CoopWave s_coop[4];
    const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i    = (long long)blockIdx.x * 256 + threadIdx.x;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (i < n) { a = ((const float4*)rays)[i * 2]; b = ((const float4*)rays)[i * 2 + 1]; }
    // the walk the DDGI and reflection passes use (trace_coop); lanes past the end of the batch only serve as triangle-test lanes
    const HitRec h = trace_coop<false, HR_ORDER_NEAR, CUTOUT>(i < n, nodes, tris, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), b.w, a.w, s_stack[wave], s_coop[wave], lane, 0u, nullptr, cv);
    if (i >= n) return;
    out_tuv[i * 3 + 0] = h.t;
    out_tuv[i * 3 + 1] = h.u;
    out_tuv[i * 3 + 2] = h.v;
    out_prim[i]        = h.prim;
}

// ---- shared instanced scenes: the queries through traverse2.h.  Kept apart from the two above: another walk (trace_coop's helper lanes there) is behaviour
template <bool CUTOUT>
__global__ __launch_bounds__(256) void k_any_hit_batch2(Scene2 sc, long long n, const float* rays, uint8_t* out, unsigned long long* stats, CutoutView cv)
{
    __shared__ uint32_t s_stack[4][HR_STACK_ENTRIES * 64];
    const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i    = (long long)blockIdx.x * 256 + threadIdx.x;
    uint32_t        nn = 0, nt = 0;
    if (i < n)
    {
        const float4 a = ((const float4*)rays)[i * 2], b = ((const float4*)rays)[i * 2 + 1];
        if constexpr (CUTOUT) out[i] = trace_any2<true>(sc, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), b.w, a.w, s_stack[wave], lane, 0u, cv) ? 1 : 0;
        else out[i] = trace2<true, true>(sc, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), b.w, a.w, s_stack[wave], lane, &nn, &nt).prim == 0 ? 1 : 0;
    }
    if (!CUTOUT && stats)
    {
        for (int o = 32; o > 0; o >>= 1) { nn += __shfl_down(nn, o); nt += __shfl_down(nt, o); }
        if (lane == 0)
        {
            atomicAdd(stats + 0, (unsigned long long)nn);
            atomicAdd(stats + 1, (unsigned long long)nt);
        }
    }
}

template <bool CUTOUT>
__global__ __launch_bounds__(256) void k_closest_hit_batch2(Scene2 sc, long long n, const float* rays, float* out_tuv, int32_t* out_prim, CutoutView cv)
{
    __shared__ uint32_t s_stack[4][HR_STACK_ENTRIES * 64];
    const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i    = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = ((const float4*)rays)[i * 2], b = ((const float4*)rays)[i * 2 + 1];
    const Hit2 h = trace_closest2<CUTOUT>(sc, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), b.w, a.w, s_stack[wave], lane, cv);
    out_tuv[i * 3 + 0] = h.t;
    out_tuv[i * 3 + 1] = h.u;
    out_tuv[i * 3 + 2] = h.v;
    out_prim[i]        = h.prim;
}

// ------------------------------------------------------------------------------------------------
// G-buffer synthesis by primary rays.  Output conventions of g_buffer.frag:86-112 (see hr_api.h).  One kernel body for every kind of scene:
// TWO_LEVEL (a shared instanced scene, instances_shared.hip) walks on two levels and makes the hit triangle's world vertices and normals at the
// hit; every other kind reads them by `prim` from the arrays its creator or its updates stored.
struct GBufArgs
{
    float           vpi[16], vp[16], pvp[16];
    float           cam[3];
    // what the walk reads comes first, what only a hit lane reads last: of the orders tried, the one with the fewest scalar-register spills around
    // the walk in all four instantiations (docs/EXPERIMENTS.md, "One G-buffer kernel body")
    const Node8*    nodes;
    const TriGPU*   tris;
    const InstanceShared* inst;    // shared scenes only: the records of the top level's leaves
    int             w, h;
    uint32_t        cull;          // shared scenes only: the HR_RAY_PRIMARY cull mask (Scene2::cull)
    uint32_t*       gb1;
    uint2*          gb2;
    uint2*          gb3;
    float*          depth;
    const float*    materials;     // [m][8] or null
    // the hit triangle's attributes.  Shared scenes: the meshes' arrays, object space, by mesh triangle; every other kind: world space, by original prim
    const float*    verts;         // [n][3][3]
    const float*    normals;       // [n][3][3] or null
    const uint32_t* tri_material;  // [n] or null
    const uint32_t* tri_mesh_id;   // [n] or null; not read for a shared scene (its mesh id is the record's)
};

// gb_pixel_dir: pixel_dir.h (k_probe_vis forms its rays with the same function)

// n, v: the hit triangle's nine world vertex-normal floats (read only where has_normals) and nine world vertex floats
HR_DEV f3 gb_normal_at(const float* n, const float* v, bool has_normals, float b0, float b1, float b2)
{
    if (has_normals) return mk3(n[0] * b0 + n[3] * b1 + n[6] * b2, n[1] * b0 + n[4] * b1 + n[7] * b2, n[2] * b0 + n[5] * b1 + n[8] * b2);
    f3 v0 = mk3(v[0], v[1], v[2]), v1 = mk3(v[3], v[4], v[5]), v2 = mk3(v[6], v[7], v[8]);
    return normalize3(cross3(sub3(v1, v0), sub3(v2, v0)));
}

HR_DEV bool gb_plane_bary(const float* v, f3 o, f3 d, float& b0, float& b1, float& b2)
{
    f3 v0 = mk3(v[0], v[1], v[2]), v1 = mk3(v[3], v[4], v[5]), v2 = mk3(v[6], v[7], v[8]);
    f3 e1 = sub3(v1, v0), e2 = sub3(v2, v0);
    f3 n  = cross3(e1, e2);
    float dn = dot3(n, d);
    if (dn == 0.0f) return false;
    float tt = __fdiv_rn(dot3(n, sub3(v0, o)), dn);
    f3    pp = sub3(add3(o, scale3(d, tt)), v0);
    float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), p1 = dot3(pp, e1), p2 = dot3(pp, e2);
    float den = d11 * d22 - d12 * d12;
    if (den == 0.0f) return false;
    b1 = __fdiv_rn(d22 * p1 - d12 * p2, den);
    b2 = __fdiv_rn(d11 * p2 - d12 * p1, den);
    b0 = 1.0f - b1 - b2;
    return true;
}

// What the MOTION instantiations read AFTER the hit, one triangle per lane (hr_gbuffer_raycast_motion): the hit triangle's previous
// world vertices are prev_verts[prim] (deformable scenes), or prev_mats[instance] * (p, 1) over the object-space positions `mesh_positions`
// (instanced kinds; a shared deformable scene passes its previous object-space positions there) — mul_m4's operation order, the bits
// k_instances_transform stores, so a matrix that stands gives the current vertices back and a delta of exactly 0.
struct MotionArgs
{
    const float*       prev_verts;       // [n][3][3] by original triangle, or null
    const float*       prev_mats;        // [n_instances][16] by instance, or null
    const InstanceRec* inst;             // private-copy scenes: the records and the triangle -> instance map
    const uint32_t*    tri_instance;
    const float*       mesh_positions;   // object space, meshes concatenated (previous frame's where they deform)
};

// previous minus current position of the point (b0, b1, b2) of a triangle: both sums in the same expression, one rounding per operation
HR_DEV f3 motion_delta(const float* vp, const float* vc, float b0, float b1, float b2)
{
    return mk3(((vp[0] * b0 + vp[3] * b1) + vp[6] * b2) - ((vc[0] * b0 + vc[3] * b1) + vc[6] * b2),
               ((vp[1] * b0 + vp[4] * b1) + vp[7] * b2) - ((vc[1] * b0 + vc[4] * b1) + vc[7] * b2),
               ((vp[2] * b0 + vp[5] * b1) + vp[8] * b2) - ((vc[2] * b0 + vc[5] * b1) + vc[8] * b2));
}
// P + delta; a delta of 0 gives P's own bits (also for a component that is -0)
HR_DEV f3 motion_prev_point(f3 P, f3 dl) { return mk3(dl.x == 0.0f ? P.x : P.x + dl.x, dl.y == 0.0f ? P.y : P.y + dl.y, dl.z == 0.0f ? P.z : P.z + dl.z); }

// m * (p, 1) for the three vertices at p: what k_instances_transform stores
HR_DEV void gb_transform_triangle(const float* m, const float* p, float* out)
{
#pragma unroll
    for (int v = 0; v < 3; v++)
    {
        const f4 w = mul_m4(m, p[v * 3], p[v * 3 + 1], p[v * 3 + 2], 1.0f);
        out[v * 3] = w.x; out[v * 3 + 1] = w.y; out[v * 3 + 2] = w.z;
    }
}

template <bool MOTION, bool TWO_LEVEL, bool CUTOUT>
__global__ __launch_bounds__(256) void k_gbuffer_raycast(GBufArgs a, MotionArgs mo, CutoutView cv)
{
    __shared__ uint32_t s_stack[4][HR_STACK_ENTRIES * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // one wave = one 8x8 tile for ray coherence
    const int tiles_x = (a.w + 7) / 8, tiles_y = (a.h + 7) / 8;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= tiles_x * tiles_y) return;
    const int x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3);
    if (x >= a.w || y >= a.h) return;
    const size_t i   = (size_t)y * a.w + x;
    const f3     cam = mk3(a.cam[0], a.cam[1], a.cam[2]);
    const f3     d   = gb_pixel_dir(a, (float)x + 0.5f, (float)y + 0.5f);
    const HitOf<TWO_LEVEL> hit = trace_closest_of<TWO_LEVEL, CUTOUT>(a.nodes, a.tris, a.inst, a.cull, cam, d, 0.0f, 1.0e30f, s_stack[wave], lane, cv);
    if (hit.prim < 0)
    {
        a.gb1[i]   = 0u;
        a.gb2[i]   = make_uint2(0u, 0u);
        a.gb3[i]   = make_uint2(0u, pack_h2(0.0f, -1.0f));
        a.depth[i] = 1.0f;
        return;
    }
    // ---- the hit triangle, the one step the kinds differ in: q, its index in verts / normals / tri_material; v and vn, its nine world vertex and
    // nine world vertex-normal floats.  A shared scene computes what k_instances_transform would have stored (model_matrix * (p, 1);
    // mat3(model_matrix) * n) into registers, through the instance record; the other kinds name the global arrays
    const bool has_normals = a.normals != nullptr;
    const InstanceShared* rec = nullptr;
    size_t       q;
    const float *v, *vn;
    float        wv[9], wn[9];
    if constexpr (TWO_LEVEL)
    {
        rec = &a.inst[hit.inst];
        q   = (size_t)rec->mesh_tri_base + hit.local;
        gb_transform_triangle(rec->m, a.verts + q * 9, wv);
        if (has_normals)
        {
            const float* n = a.normals + q * 9;
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const float nx = n[k * 3], ny = n[k * 3 + 1], nz = n[k * 3 + 2];
                wn[k * 3]     = (rec->m[0] * nx + rec->m[4] * ny) + rec->m[8] * nz;
                wn[k * 3 + 1] = (rec->m[1] * nx + rec->m[5] * ny) + rec->m[9] * nz;
                wn[k * 3 + 2] = (rec->m[2] * nx + rec->m[6] * ny) + rec->m[10] * nz;
            }
        }
        v = wv; vn = wn;
    }
    else
    {
        q  = (size_t)hit.prim;
        v  = a.verts + q * 9;
        vn = has_normals ? a.normals + q * 9 : nullptr;
    }
    const f3 P     = add3(cam, scale3(d, hit.t));
    const f4 clip  = mul_m4(a.vp, P.x, P.y, P.z, 1.0f);
    const float b0 = 1.0f - hit.u - hit.v;
    f3 Pp = P;
    if (MOTION)
    {
        float vp[9], vc[9];   // the current vertices are read before the previous state, not where motion_delta uses them
#pragma unroll
        for (int k = 0; k < 9; k++) vc[k] = v[k];
        if constexpr (TWO_LEVEL) gb_transform_triangle(mo.prev_mats + (size_t)rec->instance * 16, mo.mesh_positions + q * 9, vp);
        else if (mo.prev_verts)
        {
            const float* p = mo.prev_verts + q * 9;
#pragma unroll
            for (int k = 0; k < 9; k++) vp[k] = p[k];
        }
        else
        {
            const uint32_t     in = mo.tri_instance[q];
            const InstanceRec& r  = mo.inst[in];
            gb_transform_triangle(mo.prev_mats + (size_t)in * 16, mo.mesh_positions + ((size_t)r.mesh_tri_base + ((uint32_t)q - r.first_tri)) * 9, vp);
        }
        Pp = motion_prev_point(P, motion_delta(vp, vc, b0, hit.u, hit.v));
    }
    const f4 pclip = mul_m4(a.pvp, Pp.x, Pp.y, Pp.z, 1.0f);
    const f3 nI    = gb_normal_at(vn, v, has_normals, b0, hit.u, hit.v);
    f3       n     = normalize3(nI);
    if (dot3(n, d) > 0.0f) n = neg3(n);
    float curvature = 0.0f;
    if (has_normals)
    {
        float c0, c1, c2;
        f3    dxv = mk3(0, 0, 0), dyv = mk3(0, 0, 0);
        if (gb_plane_bary(v, cam, gb_pixel_dir(a, (float)x + 1.5f, (float)y + 0.5f), c0, c1, c2)) dxv = sub3(gb_normal_at(vn, v, true, c0, c1, c2), nI);
        if (gb_plane_bary(v, cam, gb_pixel_dir(a, (float)x + 0.5f, (float)y + 1.5f), c0, c1, c2)) dyv = sub3(gb_normal_at(vn, v, true, c0, c1, c2), nI);
        curvature = hr_sqrt(max2(dot3(dxv, dxv), dot3(dyv, dyv)));
    }
    float ox, oy;
    oct_encode(n, ox, oy);
    const float cx = __fdiv_rn(clip.x, clip.w) * 0.5f + 0.5f, cy = __fdiv_rn(clip.y, clip.w) * 0.5f + 0.5f;
    const float px = __fdiv_rn(pclip.x, pclip.w) * 0.5f + 0.5f, py = __fdiv_rn(pclip.y, pclip.w) * 0.5f + 0.5f;
    const uint32_t mat = a.tri_material ? a.tri_material[q] : 0u;
    float albedo[3] = { 0.8f, 0.8f, 0.8f }, metallic = 0.0f, roughness = 0.5f;
    if (a.materials)
    {
        const float* m = a.materials + (size_t)mat * 8;
        albedo[0] = m[0]; albedo[1] = m[1]; albedo[2] = m[2]; metallic = m[3]; roughness = m[4];
    }
    uint32_t g1 = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) g1 |= (uint32_t)(clamp1(albedo[c], 0.0f, 1.0f) * 255.0f + 0.5f) << (8 * c);
    g1 |= (uint32_t)(clamp1(metallic, 0.0f, 1.0f) * 255.0f + 0.5f) << 24;
    a.gb1[i] = g1;
    a.gb2[i] = make_uint2(pack_h2(ox, oy), pack_h2(px - cx, py - cy));
    float mesh_id;
    if constexpr (TWO_LEVEL) mesh_id = (float)rec->mesh_id;
    else mesh_id = a.tri_mesh_id ? (float)a.tri_mesh_id[q] : 0.0f;
    a.gb3[i] = make_uint2(pack_h2(max2(roughness, 0.1f), curvature), pack_h2(mesh_id, clip.z));
    const float dd = __fdiv_rn(clip.z, clip.w);
    a.depth[i] = dd >= 1.0f ? 0.99999994f : dd;
}

// hr_scene_motion_begin_frame: the instances' matrices as the device records hold them, by instance index (a shared scene's records sit in the
// order of the top level's leaves, which a re-build changes: `instance` names the row)
__global__ __launch_bounds__(256) void k_motion_snapshot_private(const InstanceRec* inst, float* prev, int n_instances)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_instances * 16) prev[i] = inst[i >> 4].m[i & 15];
}
__global__ __launch_bounds__(256) void k_motion_snapshot_shared(const InstanceShared* recs, float* prev, int n_instances)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_instances * 16) return;
    const uint32_t in = recs[i >> 4].instance;
    if (in < (uint32_t)n_instances) prev[(size_t)in * 16 + (i & 15)] = recs[i >> 4].m[i & 15];
}

// the modes of hr_selftest_math / hr_selftest_math_sweep (include/hr_api_post.h); the tests' CPU mirror restates each
HR_DEV void selftest_eval(int which, const float v[8], const SelftestParams& P, float r[SELFTEST_MAX_OUT])
{
    const float x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int k = 0; k < SELFTEST_MAX_OUT; k++) r[k] = 0.0f;
    switch (which)
    {
        case 0: det_sincos(x, r[0], r[1]); break;
        case 1: r[0] = det_exp(x); break;
        case 2: r[0] = det_log(x); break;
        case 3: r[0] = det_pow_auto(x, y); break;
        case 4: r[0] = (float)f2h(x); r[1] = h2f(f2h(x)); break;
        case 5: { f3 o = oct_decode(x, y); r[0] = o.x; r[1] = o.y; r[2] = o.z; break; }
        case 6: oct_encode(mk3(x, y, z), r[0], r[1]); break;
        case 7: r[0] = hr_sqrt(x); r[1] = __fdiv_rn(1.0f, x); break;
        case 8: r[0] = __fdiv_rn(x, y); break;
        case 9:
        {
            const DivBy D = div_prepare(y);
            r[0] = div_by(x, D);
            r[1] = div_by_inrange(x, D);
            r[2] = div_by_if(z != 0.0f, x, D);
            break;
        }
        case 10: r[0] = glsl_min(x, y); r[1] = glsl_max(x, y); r[2] = glsl_clamp(x, y, z); break;
        case 11: r[0] = min2(x, y); r[1] = max2(x, y); r[2] = clamp1(x, y, z); break;
        case 12: r[0] = mix1(x, y, z); r[1] = smoothstep1(x, y, z); r[2] = step1(x, y); r[3] = fract1(x); break;
        case 13: r[0] = det_powi(x, (y >= 0.0f && y <= 64.0f) ? (int)y : 0); r[1] = det_pow(x, y); break;
        case 14: { f3 o = world_pos_from_depth(x, y, z, P.m); r[0] = o.x; r[1] = o.y; r[2] = o.z; break; }
        case 15: r[0] = (float)(int)x; break;   // v_cvt_i32_f32 out of range (no oracle: the tests record what gfx950 does)
        default: break;
    }
}

__global__ void k_selftest_math(int which, long long n, const float* in, float* out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v[8] = { in[i * 3], in[i * 3 + 1], in[i * 3 + 2], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    SelftestParams P = {};
    float r[SELFTEST_MAX_OUT];
    selftest_eval(which, v, P, r);
    out[i * 3] = r[0]; out[i * 3 + 1] = r[1]; out[i * 3 + 2] = r[2];
}

__global__ void k_selftest_math_sweep(int which, int gen, long long first, long long n, const float* in, SelftestParams P, int nout, float* out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v[8], r[SELFTEST_MAX_OUT];
    selftest_inputs(gen, i, first, in, P, v);
    selftest_eval(which, v, P, r);
    selftest_store(i, n, nout, r, out);
}

// ------------------------------------------------------------------------------------------------
extern "C" {

hr_status hr_selftest_math(int32_t which, int64_t n, const float* in, float* out, void* stream)
{
    HR_CHECK_ARG(n >= 0 && (n == 0 || (in && out)));
    if (n == 0) return HR_OK;
    hipLaunchKernelGGL(k_selftest_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)which, (long long)n, in, out);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_selftest_math_sweep(int32_t which, int32_t gen, int64_t first, int64_t n, const float* in, const float* params, int32_t nout, float* out, void* stream)
{
    HR_CHECK_ARG(n >= 0 && params && nout >= 1 && nout <= SELFTEST_MAX_OUT && gen >= SELFTEST_GEN_ARRAY && gen <= SELFTEST_GEN_DIV);
    HR_CHECK_ARG(n == 0 || (out && (gen != SELFTEST_GEN_ARRAY || in)));
    if (n == 0) return HR_OK;
    SelftestParams P;
    std::memcpy(&P, params, sizeof(P));
    hipLaunchKernelGGL(k_selftest_math_sweep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)which, (int)gen, (long long)first,
                       (long long)n, in, P, (int)nout, out);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

const char* hr_status_string(hr_status s)
{
    switch (s)
    {
        case HR_OK: return "HR_OK";
        case HR_ERR_INVALID_ARG: return "HR_ERR_INVALID_ARG";
        case HR_ERR_HIP: return "HR_ERR_HIP";
        case HR_ERR_NO_DEVICE: return "HR_ERR_NO_DEVICE";
        case HR_ERR_OUT_OF_MEMORY: return "HR_ERR_OUT_OF_MEMORY";
        case HR_ERR_UNSUPPORTED: return "HR_ERR_UNSUPPORTED";
        case HR_ERR_TIMEOUT: return "HR_ERR_TIMEOUT";
        case HR_ERR_COMM: return "HR_ERR_COMM";
        default: return "HR_ERR_UNKNOWN";
    }
}
const char* hr_last_error(void) { return g_last_error.c_str(); }
const char* hr_version(void) { return "hybrid_rendering_amd 0.4 (gfx950)"; }
int32_t hr_api_revision(void) { return HR_API_REVISION; }

hr_status hr_ctx_create(int device_ordinal, hr_ctx** out)
{
    HR_CHECK_ARG(out);
    int        n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
    {
        set_last_error(std::string("no HIP device: ") + hipGetErrorString(e));
        return HR_ERR_NO_DEVICE;
    }
    HR_CHECK_ARG(device_ordinal >= 0 && device_ordinal < n);
    HR_HIP(hipSetDevice(device_ordinal));
    hr_ctx* c = new (std::nothrow) hr_ctx();
    if (!c) return HR_ERR_OUT_OF_MEMORY;
    c->device = device_ordinal;
    e = hipGetDeviceProperties(&c->props, device_ordinal);
    if (e != hipSuccess)
    {
        set_last_error(std::string("hipGetDeviceProperties failed: ") + hipGetErrorString(e));
        delete c;
        return HR_ERR_HIP;
    }
    *out = c;
    return HR_OK;
}

hr_status hr_ctx_destroy(hr_ctx* ctx)
{
    delete ctx;
    return HR_OK;
}

int32_t hr_ctx_device(const hr_ctx* ctx) { return ctx ? ctx->device : -1; }


static hr_status scene_create_impl(hr_ctx* ctx, const hr_scene_desc* d, hr_scene** out, bool deformable);

// Host-only: build the 8-wide BVH of a triangle soup and report its shape (no device, no upload).  What hr_scene_create
// would build for the same positions — lets an integrator (and the CPU test-suite) check depth / size limits up front.
static hr_status build_info_impl(const float* positions, int32_t n_tris, hr_scene_info* info, bool spatial, const char* call)
{
    HR_CHECK_ARG(info && n_tris >= 0 && (positions || n_tris == 0));
    return guarded(call, [&]() -> hr_status {
        BuiltBVH b;
        build_bvh8(positions, n_tris, b, spatial);
        std::memset(info, 0, sizeof(*info));
        info->n_tris     = n_tris;
        info->n_nodes    = (int32_t)b.nodes.size();
        info->max_depth  = b.max_depth;
        info->node_bytes = b.nodes.size() * sizeof(Node8);
        info->tri_bytes  = b.tris.size() * sizeof(TriGPU);
        info->box_pad    = b.pad;
        for (int a = 0; a < 3; a++) { info->bounds_lo[a] = b.lo[a]; info->bounds_hi[a] = b.hi[a]; }
        return (b.nodes.size() >= (1u << 23) || b.max_depth >= kMaxTraversalDepth) ? HR_ERR_UNSUPPORTED : HR_OK;
    });
}

hr_status hr_bvh_build_info(const float* positions, int32_t n_tris, hr_scene_info* info) { return build_info_impl(positions, n_tris, info, true, "hr_bvh_build_info"); }
// the split-free tree hr_scene_create_deformable / hr_scene_rebuild build: tri_bytes = 48 x the finite triangles
hr_status hr_bvh_build_info_deformable(const float* positions, int32_t n_tris, hr_scene_info* info) { return build_info_impl(positions, n_tris, info, false, "hr_bvh_build_info_deformable"); }

// Host-only: builds the same BVH and checks that every triangle is found from every point of its surface (bvh.h
// check_bvh8_coverage) — the invariant the spatial splits of the builder have to keep.
hr_status hr_bvh_selfcheck(const float* positions, int32_t n_tris, int32_t samples_per_triangle, int64_t* uncovered)
{
    HR_CHECK_ARG(uncovered && n_tris >= 0 && samples_per_triangle > 0 && (positions || n_tris == 0));
    return guarded("hr_bvh_selfcheck", [&]() -> hr_status {
        BuiltBVH b;
        build_bvh8(positions, n_tris, b);
        *uncovered = check_bvh8_coverage(positions, n_tris, b, samples_per_triangle);
        return HR_OK;
    });
}

// Host-only: the child boxes of the same BVH, de-quantised the way the traversal does it (origin + q * 2^(e-127), one fma per plane).
hr_status hr_bvh_child_boxes(const float* positions, int32_t n_tris, hr_child_box* out, int64_t capacity, int64_t* n_boxes)
{
    HR_CHECK_ARG(n_boxes && n_tris >= 0 && capacity >= 0 && (out || capacity == 0) && (positions || n_tris == 0));
    return guarded("hr_bvh_child_boxes", [&]() -> hr_status {
        BuiltBVH b;
        build_bvh8(positions, n_tris, b);
        std::vector<int> depth(b.nodes.size(), 0);   // children follow their parent in the builder's breadth-first order
        int64_t n = 0;
        for (size_t j = 0; j < b.nodes.size(); j++)
        {
            const Node8& nd = b.nodes[j];
            const int n_internal = nd.counts & 15, n_children = nd.counts >> 4;
            for (int c = 0; c < n_internal; c++) depth[(size_t)nd.child_base + c] = depth[j] + 1;
            const uint8_t e[3] = { nd.ex, nd.ey, nd.ez };
            const float   o[3] = { nd.ox, nd.oy, nd.oz };
            for (int c = 0; c < n_children; c++, n++)
            {
                if (n >= capacity) continue;
                hr_child_box& r = out[n];
                for (int a = 0; a < 3; a++)
                {
                    const uint32_t bits = (uint32_t)e[a] << 23;
                    float step;
                    std::memcpy(&step, &bits, 4);
                    r.step[a] = step;
                    r.lo[a] = std::fma((float)nd.qlo[a][c], step, o[a]);
                    r.hi[a] = std::fma((float)nd.qhi[a][c], step, o[a]);
                }
                r.node = (int32_t)j; r.slot = c; r.depth = depth[j]; r.is_leaf = c >= n_internal ? 1 : 0;
            }
        }
        *n_boxes = n;
        return HR_OK;
    });
}

hr_status hr_scene_create(hr_ctx* ctx, const hr_scene_desc* d, hr_scene** out)
{
    return guarded("hr_scene_create", [&] { return scene_create_impl(ctx, d, out, false); });
}

static hr_status scene_create_impl(hr_ctx* ctx, const hr_scene_desc* d, hr_scene** out, bool deformable)
{
    HR_CHECK_ARG(ctx && d && out && d->n_tris >= 0 && (d->positions || d->n_tris == 0));
    HR_CHECK_ARG(d->n_materials >= 0 && (d->materials || d->n_materials == 0));
    if (d->tri_material)
    {
        if (!d->materials) { set_last_error("hr_scene_create: tri_material given without materials"); return HR_ERR_INVALID_ARG; }
        const int i = first_bad_material(d->tri_material, d->n_tris, d->n_materials);
        if (i >= 0)
        {
            set_last_error("hr_scene_create: tri_material[" + std::to_string(i) + "] = " + std::to_string(d->tri_material[i]) + " >= n_materials");
            return HR_ERR_INVALID_ARG;
        }
    }
    HR_HIP(hipSetDevice(ctx->device));
    BuiltBVH b;
    build_bvh8(d->positions, d->n_tris, b, !deformable);
    if (b.nodes.size() >= (1u << 23))   // traversal stack entries hold child_base in 23 bits
    {
        set_last_error("hr_scene_create: more than 2^23 BVH nodes");
        return HR_ERR_UNSUPPORTED;
    }
    if (b.tris.size() >= kCoopMaxTriangles)   // cooperative triangle jobs hold the triangle reference in 26 bits (traverse.h CoopWave)
    {
        set_last_error("hr_scene_create: more than 2^26 triangle references");
        return HR_ERR_UNSUPPORTED;
    }
    if (b.max_depth >= kMaxTraversalDepth)   // one stack entry per level (traverse.h); the builder's depth cap keeps real input below it
    {
        set_last_error("hr_scene_create: BVH depth " + std::to_string(b.max_depth) + " exceeds the traversal stack (" + std::to_string(kMaxTraversalDepth) + ")");
        return HR_ERR_UNSUPPORTED;
    }
    std::unique_ptr<hr_scene> guard(new hr_scene());
    hr_scene* s = guard.get();
    s->ctx      = ctx;
    HR_TRY(upload(s->nodes, b.nodes.data(), b.nodes.size() * sizeof(Node8)));
    HR_TRY(upload(s->tris, b.tris.data(), b.tris.size() * sizeof(TriGPU)));
    const size_t n = (size_t)d->n_tris;
    if (d->normals) { HR_TRY(upload(s->tri_normals, d->normals, n * 36)); s->has_normals = true; }
    if (d->tri_material) { HR_TRY(upload(s->tri_material, d->tri_material, n * 4)); s->has_material = true; }
    if (d->tri_mesh_id) { HR_TRY(upload(s->tri_mesh_id, d->tri_mesh_id, n * 4)); s->has_mesh_id = true; }
    HR_TRY(upload(s->positions, d->positions, n * 36));   // original-order vertex positions are kept for shading-time interpolation
    HR_TRY(stage_materials(s, d, "hr_scene_create"));
    if (s->has_textures)
    {
        if (d->uvs) { HR_TRY(upload(s->tri_uvs, d->uvs, n * 24)); s->has_uvs = true; }
        if (d->tangents) { HR_TRY(upload(s->tri_tangents, d->tangents, n * 36)); s->has_tangents = true; }
    }
    { static std::atomic<uint64_t> next_uid { 1 }; s->uid = next_uid.fetch_add(1); }
    s->info.n_tris      = d->n_tris;
    s->info.n_nodes     = (int32_t)b.nodes.size();
    s->info.max_depth   = b.max_depth;
    s->info.node_bytes  = b.nodes.size() * sizeof(Node8);
    s->info.tri_bytes   = b.tris.size() * sizeof(TriGPU);
    s->info.box_pad     = b.pad;
    for (int a = 0; a < 3; a++) { s->info.bounds_lo[a] = s->grid_lo[a] = b.lo[a]; s->info.bounds_hi[a] = s->grid_hi[a] = b.hi[a]; }
    if (deformable) HR_TRY(deformable_scene_adopt(s, b));
    *out = guard.release();
    return HR_OK;
}

// nearest-filtered mip level of the four G-buffer images (g_buffer.cpp:240-243: vkCmdBlitImage, VK_FILTER_NEAREST):
// destination texel (x, y) = source texel (x << level, y << level)
__global__ __launch_bounds__(256) void k_gbuffer_mip(hr_gbuffer_level src, hr_gbuffer_level dst, int level)
{
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= dst.width || y >= dst.height) return;
    const size_t so = (size_t)(y << level) * src.width + (x << level), o = (size_t)y * dst.width + x;
    if (src.gb1 && dst.gb1) ((uint32_t*)dst.gb1)[o] = ((const uint32_t*)src.gb1)[so];
    ((uint2*)dst.gb2)[o] = ((const uint2*)src.gb2)[so];
    ((uint2*)dst.gb3)[o] = ((const uint2*)src.gb3)[so];
    ((float*)dst.depth)[o] = src.depth[so];
}

extern "C" hr_status hr_gbuffer_mip_nearest(const hr_gbuffer_level* src, const hr_gbuffer_level* dst, int32_t level, void* stream)
{
    HR_CHECK_ARG(src && dst && level >= 1 && level <= 8 && src->gb2 && src->gb3 && src->depth && dst->gb2 && dst->gb3 && dst->depth);
    HR_CHECK_ARG(dst->width == (src->width >> level) && dst->height == (src->height >> level) && dst->width > 0 && dst->height > 0);
    hipLaunchKernelGGL(k_gbuffer_mip, dim3(cdiv(dst->width, 32), cdiv(dst->height, 8)), dim3(256), 0, (hipStream_t)stream, *src, *dst, (int)level);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_scene_get_info(const hr_scene* scene, hr_scene_info* info)
{
    HR_CHECK_ARG(scene && info);
    if (scene->n_instances > 0 && !scene->shared)   // a shared scene transforms no vertex: its bounds are the host's conservative ones
    {
        const hr_status s = instanced_scene_refresh_bounds(scene);   // the exact bounds of the last hr_scene_update_instances, read back on demand
        if (s != HR_OK) return s;
    }
    if (scene->deformable)
    {
        const hr_status s = deformable_scene_refresh_bounds(scene);   // the exact bounds of the last hr_scene_update_vertices
        if (s != HR_OK) return s;
    }
    *info = scene->info;
    return HR_OK;
}

uint64_t hr_scene_id(const hr_scene* scene) { return scene ? scene->uid : 0; }

hr_status hr_scene_read_bvh(const hr_scene* scene, void* nodes_out, void* tris_out)
{
    HR_CHECK_ARG(scene);
    HR_HIP(hipSetDevice(scene->ctx->device));
    HR_HIP(hipDeviceSynchronize());
    if (nodes_out) HR_HIP(hipMemcpy(nodes_out, scene->nodes.p, (size_t)scene->info.node_bytes, hipMemcpyDeviceToHost));
    if (tris_out) HR_HIP(hipMemcpy(tris_out, scene->tris.p, (size_t)scene->info.tri_bytes, hipMemcpyDeviceToHost));
    return HR_OK;
}

hr_status hr_scene_destroy(hr_scene* scene)
{
    if (scene)
    {
        (void)hipSetDevice(scene->ctx->device);
        (void)hipDeviceSynchronize();
        delete scene;
    }
    return HR_OK;
}

hr_status hr_trace_any_hit(const hr_scene* scene, int64_t n, const float* rays, uint8_t* out, uint64_t* stats, void* stream)
{
    HR_CHECK_ARG(scene && n >= 0 && (n == 0 || (rays && out)));
    HR_REJECT_CUTOUT(scene, HR_RAY_QUERY, "hr_trace_any_hit", stats != nullptr);
    if (n == 0) return HR_OK;
    const bool       cutout = cutout_on(scene, HR_RAY_QUERY);
    const CutoutView cv = cutout ? cutout_view_of(scene) : CutoutView();
    if (scene->shared)
    {
        hipLaunchKernelGGL(cutout ? k_any_hit_batch2<true> : k_any_hit_batch2<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scene2_of(scene, HR_RAY_QUERY), (long long)n, rays, out, (unsigned long long*)stats, cv);
        HR_HIP(hipGetLastError());
        return HR_OK;
    }
    hipLaunchKernelGGL(cutout ? k_any_hit_batch<true> : k_any_hit_batch<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const Node8*)scene->nodes.p,
                       (const TriGPU*)scene->tris.p, (long long)n, rays, out, (unsigned long long*)stats, cv);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_trace_closest_hit(const hr_scene* scene, int64_t n, const float* rays, float* out_tuv, int32_t* out_prim, void* stream)
{
    HR_CHECK_ARG(scene && n >= 0 && (n == 0 || (rays && out_tuv && out_prim)));
    if (n == 0) return HR_OK;
    const bool       cutout = cutout_on(scene, HR_RAY_QUERY);
    const CutoutView cv = cutout ? cutout_view_of(scene) : CutoutView();
    if (scene->shared)
    {
        hipLaunchKernelGGL(cutout ? k_closest_hit_batch2<true> : k_closest_hit_batch2<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scene2_of(scene, HR_RAY_QUERY), (long long)n, rays, out_tuv, out_prim, cv);
        HR_HIP(hipGetLastError());
        return HR_OK;
    }
    hipLaunchKernelGGL(cutout ? k_closest_hit_batch<true> : k_closest_hit_batch<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const Node8*)scene->nodes.p,
                       (const TriGPU*)scene->tris.p, (long long)n, rays, out_tuv, out_prim, cv);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

// motion: hr_gbuffer_raycast_motion on a scene that holds a previous state (a flat scene has none: nothing of it ever moves)
static hr_status gbuffer_raycast_impl(const hr_scene* scene, const hr_ubo* ubo, int32_t w, int32_t h, void* gb1, void* gb2, void* gb3, float* depth, void* stream, bool motion)
{
    HR_CHECK_ARG(scene && ubo && w > 0 && h > 0 && gb1 && gb2 && gb3 && depth);
    motion = motion && scene->motion && (scene->n_instances > 0 || scene->deformable);
    MotionArgs mo = { nullptr, nullptr, nullptr, nullptr, nullptr };
    if (motion)
    {
        if (scene->n_instances > 0)
        {
            mo.prev_mats = (const float*)scene->prev_mats.p;
            mo.inst = (const InstanceRec*)scene->inst_records.p; mo.tri_instance = (const uint32_t*)scene->tri_instance.p;
            mo.mesh_positions = (const float*)(scene->deform ? scene->prev_positions.p : scene->mesh_positions.p);
        }
        else mo.prev_verts = (const float*)scene->prev_positions.p;
    }
    // a shared scene's attribute arrays are its meshes' (object space); the hit makes world vertices and normals of them
    const bool sh = scene->shared;
    GBufArgs a;
    for (int i = 0; i < 16; i++) { a.vpi[i] = ubo->view_proj_inverse[i]; a.vp[i] = ubo->view_proj[i]; a.pvp[i] = ubo->prev_view_proj[i]; }
    for (int i = 0; i < 3; i++) a.cam[i] = ubo->cam_pos[i];
    a.nodes = (const Node8*)scene->nodes.p; a.tris = (const TriGPU*)scene->tris.p;
    a.inst = sh ? (const InstanceShared*)scene->inst_shared.p : nullptr;
    a.cull = cull_of(scene, HR_RAY_PRIMARY);
    a.normals = scene->has_normals ? (const float*)(sh ? scene->mesh_normals.p : scene->tri_normals.p) : nullptr;
    a.tri_material = scene->has_material ? (const uint32_t*)(sh ? scene->mesh_material.p : scene->tri_material.p) : nullptr;
    a.tri_mesh_id = scene->has_mesh_id && !sh ? (const uint32_t*)scene->tri_mesh_id.p : nullptr;
    a.materials = scene->n_materials ? (const float*)scene->materials.p : nullptr;
    a.verts = (const float*)(sh ? scene->mesh_positions.p : scene->positions.p);
    a.w = w; a.h = h;
    a.gb1 = (uint32_t*)gb1; a.gb2 = (uint2*)gb2; a.gb3 = (uint2*)gb3; a.depth = depth;
    const int tiles = ((w + 7) / 8) * ((h + 7) / 8);
    // a private-copy instanced scene never enables cutouts (cutout.hip scene_check)
    const bool       cutout = cutout_on(scene, HR_RAY_PRIMARY);
    const CutoutView cv = cutout ? cutout_view_of(scene) : CutoutView();
    void (*const kernel[2][2][2])(GBufArgs, MotionArgs, CutoutView) = { { { k_gbuffer_raycast<false, false, false>, k_gbuffer_raycast<false, false, true> }, { k_gbuffer_raycast<false, true, false>, k_gbuffer_raycast<false, true, true> } },
                                                                        { { k_gbuffer_raycast<true, false, false>, k_gbuffer_raycast<true, false, true> }, { k_gbuffer_raycast<true, true, false>, k_gbuffer_raycast<true, true, true> } } };
    hipLaunchKernelGGL(kernel[motion][sh][cutout], dim3((tiles + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, mo, cv);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_gbuffer_raycast(const hr_scene* scene, const hr_ubo* ubo, int32_t w, int32_t h, void* gb1, void* gb2, void* gb3, float* depth, void* stream)
{
    return gbuffer_raycast_impl(scene, ubo, w, h, gb1, gb2, gb3, depth, stream, false);
}

hr_status hr_gbuffer_raycast_motion(const hr_scene* scene, const hr_ubo* ubo, int32_t w, int32_t h, void* gb1, void* gb2, void* gb3, float* depth, void* stream)
{
    return gbuffer_raycast_impl(scene, ubo, w, h, gb1, gb2, gb3, depth, stream, true);
}

// The snapshot of a frame's geometry, on `stream`: the instances' matrices out of the DEVICE records (they hold what the updates enqueued so far
// on that stream, whatever the host mirrors say by now), the vertices by device copies.  O(instances) for the instanced kinds, 36 B per triangle
// for a deformable scene, 36 B per triangle of the flagged meshes more for a shared deformable one.
hr_status hr_scene_motion_begin_frame(hr_scene* scene, void* stream)
{
    HR_CHECK_ARG(scene);
    hr_scene* s = scene;
    if (s->n_instances <= 0 && !s->deformable) return HR_OK;   // hr_scene_create: nothing of it ever moves
    hipStream_t st = (hipStream_t)stream;
    HR_HIP(hipSetDevice(s->ctx->device));
    const bool first = !s->motion;
    hr_status e;
    if (s->n_instances > 0)
    {
        const int I = s->n_instances;
        if (first && (e = s->prev_mats.alloc((size_t)I * 64)) != HR_OK) return e;
        if (s->shared) hipLaunchKernelGGL(k_motion_snapshot_shared, dim3(cdiv(I * 16, 256)), dim3(256), 0, st, (const InstanceShared*)s->inst_shared.p, (float*)s->prev_mats.p, I);
        else hipLaunchKernelGGL(k_motion_snapshot_private, dim3(cdiv(I * 16, 256)), dim3(256), 0, st, (const InstanceRec*)s->inst_records.p, (float*)s->prev_mats.p, I);
        HR_HIP(hipGetLastError());
        if (s->deform)
        {
            const hr::DeformRefit& sd = *s->deform;
            if (first)
            {
                // the whole array once (the kernel indexes it like mesh_positions); afterwards only the meshes that can change
                if ((e = s->prev_positions.alloc(s->mesh_positions.bytes)) != HR_OK) return e;
                HR_HIP(hipMemcpyAsync(s->prev_positions.p, s->mesh_positions.p, s->mesh_positions.bytes, hipMemcpyDeviceToDevice, st));
            }
            else
                for (size_t k = 0; k < sd.flag.size(); k++)
                {
                    const size_t off = (size_t)sd.tri_base[k] * 36, n = (size_t)sd.n_tris[k] * 36;
                    if (!sd.flag[k] || n == 0 || off + n > s->prev_positions.bytes) continue;
                    HR_HIP(hipMemcpyAsync((char*)s->prev_positions.p + off, (const char*)s->mesh_positions.p + off, n, hipMemcpyDeviceToDevice, st));
                }
        }
    }
    else
    {
        const size_t n = (size_t)s->info.n_tris * 36;
        if (first && (e = s->prev_positions.alloc(n)) != HR_OK) return e;
        if (n > 0) HR_HIP(hipMemcpyAsync(s->prev_positions.p, s->positions.p, n, hipMemcpyDeviceToDevice, st));
    }
    s->motion = true;
    return HR_OK;
}

} // extern "C"

hr_status hr::scene_create_flat(hr_ctx* ctx, const hr_scene_desc* d, hr_scene** out, bool deformable) { return scene_create_impl(ctx, d, out, deformable); }
