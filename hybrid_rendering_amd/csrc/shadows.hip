// RayTracedShadows on MI355X — HIP replacement for src/ray_traced_shadows.{h,cpp} and
// src/shaders/shadows/*.  Stage map (reference file:line -> kernel):
//   ray_trace()              ray_traced_shadows.cpp:972-1011, shadows_ray_trace.comp:89-132   -> k_shadows_trace
//   reset_args()+temporal()  :1015-1090, shadows_denoise_reprojection.comp:196-293            -> k_shadows_temporal
//   a_trous_filter()         :1094-1215, shadows_denoise_atrous.comp:94-174 +
//                            shadows_denoise_copy_shadow_tiles.comp:32-36 (fused via tile class) -> k_shadows_atrous
//   upsample()               :1219-1255, shadows_upsample.comp:62-109                          -> k_upsample (upsample.h)
#include "hr_internal.h"
#include "reproject.h"
#include "traverse.h"
#include "traverse2.h"
#include "shading.h"
#include "cutout_host.h"
#include "upsample.h"
#include "pass_args.h"
#include "tile_order.h"
#include "pass_core.h"

using namespace hr;

// ------------------------------------------------------------------------------------------------
struct TraceArgs
{
    float           vpi[16];
    hr_light        light;
    const float*    depth;
    const uint2*    gb2;
    const uint8_t*  sobol;
    const uint8_t*  sr;
    uint32_t*       mask;
    uint16_t*       ray_slots;  // rays fired per 8x8 tile (no shared atomic counter: one contended address serialised ~13 ns per wave)
    const Node8*    nodes;
    const TriGPU*   tris;
    unsigned long long* stats; // nullable: [0] nodes visited, [1] triangles tested
    unsigned long long* timeline; // nullable (HR_DEBUG_TIMELINE): per tile {start, end} in 100 MHz ticks + hw id
    int             w, h;      // pass image (full frame)
    int             y0, y1;    // resident rows
    int             mw;        // mask words per row
    int             tiles_x, tiles_y, tile_y0, debug_skip_traversal, debug_only_tx, debug_only_ty;
    float           bias;
    uint32_t        num_frames;
    uint32_t*       occluder;  // nullable: per pixel, the index (into tris) of the triangle that occluded its ray last frame (see k_shadows_trace)
    uint32_t        n_tri_refs;
    const uint32_t* order;     // nullable: launch slot -> tile, heaviest tiles of the last frame first (tile_order.h)
    uint16_t*       cost;      // nullable: per tile, how long its wave lived (100 MHz ticks)
    const InstanceShared* inst; // SHARED only: one record per top-level leaf (instances_shared.hip); last, so that no other member moves
    uint32_t        cull;       // SHARED only: the scene's HR_RAY_SHADOW cull mask (Scene2::cull)
};

// One wave = one 8x8 pixel tile = two 8x4 mask words; lane l -> pixel (l & 7, l >> 3), so the
// wave ballot IS the packed mask (bit y*8+x of shadows_ray_trace.comp:126).
#define TRACE_WAVES 1 // waves (8x8 tiles) per workgroup: 1 lets the dispatcher back-fill a CU wave by wave — tile
                      // costs differ by >10x, and with 4-wave groups the finished waves' slots idle until the slowest ends
#ifndef SHADOWS_TRACE_EU
#define SHADOWS_TRACE_EU 1   // minimum waves per SIMD the register allocator must leave room for (A/B: see docs/EXPERIMENTS.md R4.3)
#endif
// SHARED: over a shared instanced scene (instances_shared.hip) — the same pixel -> ray set-up, the two-level walk of traverse2.h.  The occluder
// cache is off there (it stores an index into a world-space `tris`; the mask does not depend on it), and so are the developer switches and the
// timeline, which the host refuses on such a scene.  <STATS, false> is the kernel as it was.
// CUTOUT: the walk and the occluder cache's early test run the alpha test (cutout.h) through `cv`, so only an ACCEPTED triangle answers or is cached;
// the host picks it iff cutout_on(scene, HR_RAY_SHADOW).  `cv` is unset and unread otherwise.
template <bool STATS, bool SHARED = false, bool CUTOUT = false>
__global__ __launch_bounds__(64 * TRACE_WAVES, SHADOWS_TRACE_EU) void k_shadows_trace(TraceArgs a, CutoutView cv)
{
    static_assert(!(STATS && SHARED), "no statistics build of the two-level walk");
    static_assert(!(STATS && CUTOUT), "no statistics build of the cutout walks");
    __shared__ uint32_t s_stack[TRACE_WAVES][HR_STACK_ENTRIES * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int launch_slot = blockIdx.x * TRACE_WAVES + wave;
    if (launch_slot >= a.tiles_x * a.tiles_y) return;
    // Tile order: row-major, or last frame's heaviest tiles first (tile_order.h).  Stride permutations lose BVH locality in L2.
    const int slot = a.order ? (int)a.order[launch_slot] : launch_slot;
    const int tx = slot % a.tiles_x, ty_local = slot / a.tiles_x, ty = ty_local + a.tile_y0;
    if constexpr (!SHARED)
        if (a.debug_only_tx >= 0 && (tx != a.debug_only_tx || ty != a.debug_only_ty)) return;
    unsigned long long t_begin = 0;
    if ((!SHARED && a.timeline) || a.cost) t_begin = wall_clock64();
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    bool      lit = false, fired = false;
    uint32_t  nn = 0, nt = 0, wave_max = 0;
    // depth, normal and blue-noise texel of the pixel in ONE round trip (a lane outside the image reads a valid address and
    // ignores the values) instead of depth -> normal -> noise one after the other
    const int    kind = trace_lane_kind(x, y, a.w, a.h, a.y0, a.y1);
    const size_t pix  = kind == 1 ? (size_t)y * a.w + x : (size_t)a.y0 * a.w;
    const float    d_pre  = a.depth[pix];
    const uint2    g2_pre = a.gb2[pix];
    const uint32_t bn_pre = blue_noise_texel(x, y, a.sr);
    uint32_t occ_pre = 0xffffffffu;
    if constexpr (!SHARED) occ_pre = a.occluder ? a.occluder[pix] : 0xffffffffu;
    if (kind)
    {
        const float d = kind == 1 ? d_pre : 0.0f;      // edge thread: out-of-image fetches read 0
        if (d != 1.0f)
        {
            const float tu = __fdiv_rn((float)x + 0.5f, (float)a.w), tv = __fdiv_rn((float)y + 0.5f, (float)a.h);
            const f3    P  = world_pos_from_depth(tu, tv, d, a.vpi);
            const uint2 g2 = kind == 1 ? g2_pre : make_uint2(0u, 0u);
            const f3    N  = oct_decode(h2f_lo(g2.x), h2f_hi(g2.x));
            const f3    ro = add3(P, scale3(N, a.bias));
            const float r0 = sample_blue_noise_t(bn_pre, (int)a.num_frames, 0, a.sobol);
            const float r1 = sample_blue_noise_t(bn_pre, (int)a.num_frames, 1, a.sobol);
            f3    Wi;
            float t_max, att;
            fetch_light_shadow(a.light, P, N, r0, r1, Wi, t_max, att);
            if (att > 0.0f)
            {
                fired = true;
                if constexpr (SHARED) lit = !trace_any2<CUTOUT>({ a.nodes, a.tris, a.inst, a.cull }, ro, Wi, 0.01f, t_max, s_stack[wave], lane, 0u, cv);
                else
                {
                    // Occluder cache: "is ANY triangle hit in (t_min, t_max)" is a pure function of the geometry, so testing one particular
                    // triangle FIRST and answering "occluded" when it is hit cannot change the mask — and the triangle that shadowed this
                    // pixel last frame (static light, camera moving a fraction of a pixel) shadows it again almost always.  66 % of the bench
                    // frame's shadow rays are occluded; a tile whose lanes are all answered by their cached triangle skips the walk, and in
                    // mixed tiles the occluded lanes (the ones that would otherwise walk until their first hit) drop out of the wave's
                    // longest-lane race.  A stale or foreign index is harmless: the CURRENT scene's triangle at that index is tested.
                    bool occluded = false;
                    uint32_t hit_tri = 0xffffffffu;
                    if (a.occluder && kind == 1 && !a.debug_skip_traversal)
                    {
                        const uint32_t c = occ_pre;
                        if (c < a.n_tri_refs)
                        {
                            const RayPre rp = ray_prepare(ro, Wi);
                            float t, u, v;
                            const TriRaw tc = load_tri_raw(a.tris, c);
                            occluded = ray_tri_raw<CUTOUT>(rp, tc, 0.01f, t_max, t, u, v);
                            if (CUTOUT) occluded = occluded && cutout_accept(cv, tc.a.w, u, v);
                            if (STATS) nt++;
                            hit_tri = c;
                        }
                    }
                    if (a.debug_skip_traversal) lit = (ro.x + Wi.y > -1e30f);
                    else if (!occluded)
                    {
                        hit_tri = 0xffffffffu;
                        occluded = trace_any<STATS, HR_ANY_ORDER, CUTOUT>(a.nodes, a.tris, ro, Wi, 0.01f, t_max, s_stack[wave], lane, nn, nt, 0u, nullptr, &hit_tri, cv);
                    }
                    if (!a.debug_skip_traversal) lit = !occluded;
                    if (a.occluder && kind == 1 && hit_tri != occ_pre) a.occluder[pix] = hit_tri;
                }
            }
        }
    }
    const unsigned long long bits = __ballot(lit);
    const unsigned long long fb   = __ballot(fired);
    if (STATS)
    {
        // wave reduction of the counters
        uint32_t mx = nn + nt; // per-lane traversal steps; the wave runs until its slowest lane is done
        for (int o = 32; o > 0; o >>= 1) { uint32_t t = __shfl_down(mx, o); mx = t > mx ? t : mx; }
        wave_max = mx;
        for (int o = 32; o > 0; o >>= 1) { nn += __shfl_down(nn, o); nt += __shfl_down(nt, o); }
    }
    if (lane == 0)
    {
        const int my = ty * 2;
        if (my * 4 >= a.y0 && my * 4 < a.y1) a.mask[(size_t)my * a.mw + tx] = (uint32_t)(bits & 0xffffffffull);
        if ((my + 1) * 4 >= a.y0 && (my + 1) * 4 < a.y1 && (my + 1) * 4 < a.h) a.mask[(size_t)(my + 1) * a.mw + tx] = (uint32_t)(bits >> 32);
        a.ray_slots[(size_t)ty * a.tiles_x + tx] = (uint16_t)__popcll(fb);
        if (a.cost)
        {
            const unsigned long long ticks = wall_clock64() - t_begin;
            a.cost[slot] = (uint16_t)(ticks > 65535ull ? 65535ull : ticks);
        }
        if (!SHARED && a.timeline)
        {
            const unsigned long long t_end = wall_clock64();
            uint32_t hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            uint32_t xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            a.timeline[(size_t)slot * 4 + 0] = t_begin;
            a.timeline[(size_t)slot * 4 + 1] = t_end;
            a.timeline[(size_t)slot * 4 + 2] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
            a.timeline[(size_t)slot * 4 + 3] = (unsigned long long)wave_max | ((unsigned long long)(nn + nt) << 32); // STATS build only
        }
        if (STATS && a.stats)
        {
            atomicAdd(a.stats + 0, (unsigned long long)nn);
            atomicAdd(a.stats + 1, (unsigned long long)nt);
            atomicAdd(a.stats + 2, (unsigned long long)wave_max);
        }
    }
}

// ------------------------------------------------------------------------------------------------

#ifndef TEMPORAL_WAVES
#define TEMPORAL_WAVES 4
#endif
__global__ __launch_bounds__(64 * TEMPORAL_WAVES) void k_shadows_temporal(TemporalArgs a)
{
    __shared__ uint32_t s_mask[TEMPORAL_WAVES][18];
    __shared__ uint32_t s_rows[TEMPORAL_WAVES][24];
    __shared__ float    s_vpi[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * TEMPORAL_WAVES + wave;
    const bool tile_ok = tile < a.tiles_x * a.tiles_y;
    const int tx = tile_ok ? tile % a.tiles_x : 0, ty = (tile_ok ? tile / a.tiles_x : 0) + a.tile_y0;
    if (threadIdx.x < 16) s_vpi[threadIdx.x] = a.vpi[threadIdx.x];
    if (tile_ok && lane < 18)
    {
        // populate_cache (:114-123): 3x6 masks around the tile; out-of-image masks read 0 (pinned)
        const int cx = tx - 1 + lane % 3, cy = ty * 2 - 2 + lane / 3;
        uint32_t  v  = 0u;
        if (cx >= 0 && cy >= 0 && cx < a.mw && cy < a.mh && cy * 4 >= a.y0 - 8 && cy * 4 < a.y1 + 8) v = a.mask[(size_t)cy * a.mw + cx];
        s_mask[wave][lane] = v;
    }
    __syncthreads();
    const int lx = lane & 7, ly = lane >> 3;
    const int x = tx * 8 + lx, y = ty * 8 + ly;

    // 17x17 box sum of visibility bits (neighborhood_mean :157-190): integer popcounts are exact.
    // The 24-bit row patterns of the 24 cached pixel rows are the same for every lane of the wave: lanes 0..23 build
    // one each (3 byte extracts) into LDS, then every lane popcounts its 17-row x 17-bit window.
    if (lane < 24)
    {
        const int m = lane >> 2, br = lane & 3;
        const uint32_t w0 = s_mask[wave][m * 3 + 0], w1 = s_mask[wave][m * 3 + 1], w2 = s_mask[wave][m * 3 + 2];
        s_rows[wave][lane] = ((w0 >> (br * 8)) & 0xffu) | (((w1 >> (br * 8)) & 0xffu) << 8) | (((w2 >> (br * 8)) & 0xffu) << 16);
    }
    __syncthreads();
    int sum = 0;
#pragma unroll
    for (int yy = 0; yy <= 16; yy++) sum += __popc((s_rows[wave][ly + yy] >> lx) & 0x1ffffu);
    if (!tile_ok) return;
    const float mean = __fdiv_rn((float)sum, 289.0f);

    const bool in_image = x < a.w && y < a.h && y >= a.y0 && y < a.y1;
    // A thread right of / below a ragged image has no pixel, but the shader has no bounds check (:196-293): it reads depth 0
    // and G-buffer 0 (pinned out-of-image fetch), runs the body (its stores are dropped) and still votes in
    // g_should_denoise — e.g. with the mask bit its twin in the ray-trace dispatch produced (device_math.h trace_lane_kind).
    const bool edge = x >= a.w || y >= a.h;
    float      out_v = 0.0f, out_var = 0.0f, m0 = 0.0f, m1 = 0.0f, hlen = 0.0f;
    bool       flag = false, apron_miss = false;
    if (in_image || edge)
    {
        const size_t pix = in_image ? (size_t)y * a.w + x : (size_t)a.y0 * a.w;
        const float d = edge ? 0.0f : a.depth.p[pix];
        // centre G-buffer texel: fetched and decoded ONCE, for the reprojection and for the a-trous iterations (nd)
        const uint2 cg2 = edge ? make_uint2(0u, 0u) : a.gb2.p[pix], cg3 = edge ? make_uint2(0u, 0u) : a.gb3.p[pix];
        const f3    cn  = oct_decode(h2f_lo(cg2.x), h2f_hi(cg2.x));
        if (d != 1.0f)
        {
            const int   cry = ly + 8, crx = lx + 8;
            const float visibility = (float)((s_mask[wave][(cry >> 2) * 3 + (crx >> 3)] >> ((cry & 3) * 8 + (crx & 7))) & 1u);
            ReprojIn in;
            in.x = x; in.y = y; in.depth = d; in.vpi = a.vpi; // kernel argument => scalar registers
            in.gb2 = a.gb2; in.gb3 = a.gb3; in.pgb2 = a.pgb2; in.pgb3 = a.pgb3; in.pdepth = a.pdepth;
            in.w = a.w; in.h = a.h;
            in.has_center = true; in.c2 = cg2; in.c3 = cg3; in.cur_n = cn;
            float hv, hm[2];
            ImgR16F none { nullptr, 0, 0, 0 };
            bool success = false;
            if (!a.debug_skip_reproject) success = reproject<true, true, false, ImgRG16F>(in, a.hist, a.hist_moments, none, &hv, hm, hlen);
            else { hv = 0.0f; hm[0] = hm[1] = 0.0f; hlen = 0.0f; }
            apron_miss = in.apron_miss && in_image && y >= a.band_y0 && y < a.band_y1;
            hlen = min2(32.0f, success ? hlen + 1.0f : 1.0f);
            if (success)
            {
                float sv = max2(mean - mean * mean, 0.0f);
                float sd = hr_sqrt(sv);
                hv       = clamp1(hv, mean - 0.5f * sd, mean + 0.5f * sd);
            }
            const float al = success ? max2(a.alpha, __fdiv_rn(1.0f, hlen)) : 1.0f;
            const float am = success ? max2(a.moments_alpha, __fdiv_rn(1.0f, hlen)) : 1.0f;
            m0      = visibility;
            m1      = m0 * m0;
            m0      = mix1(hm[0], m0, am);
            m1      = mix1(hm[1], m1, am);
            out_var = max2(0.0f, m1 - m0 * m0);
            out_v   = mix1(hv, visibility, al);
            flag    = out_v > 0.0f;
        }
        if (in_image)
        {
            a.out_moments[pix] = make_uint2(pack_h2(m0, m1), pack_h2(hlen, 0.0f));
            // the a-trous iterations read every pixel's normal 9x4 times: store the decoded one
            a.nd[pix]  = make_float4(cn.x, cn.y, cn.z, h2f_hi(cg3.y));
            a.out[pix] = pack_h2(out_v, out_var);
        }
    }
    if (a.apron_flag && __ballot(apron_miss) && lane == 0) atomicOr(a.apron_flag, 1u);
    // tile classification (:275-291): any lit pixel => the tile needs the à-trous filter
    const unsigned long long any = __ballot(flag);
    if (lane == 0) a.tile_class[(size_t)ty * a.tiles_x + tx] = any ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------

// edge_stopping.glsl:31-62 with NORMAL + LUMA weights.  FAST = the reference's default parameters
// (phi_normal == 32, sigma_depth == 1): x / 1.0f == x and pow(x, 32) is five squarings — same bits, fewer ops.
template <bool FAST>
HR_DEV float edge_weight(float cd, float sd, float phi_z, f3 cn, f3 sn, float phi_n, float cl, float sl, const DivBy& phi_l)
{
    const float dz = -fabsf(cd - sd);
    const float wZ = det_exp(FAST ? dz : __fdiv_rn(dz, phi_z));
    const float dn = clamp1(dot3(cn, sn), 0.0f, 1.0f);
    float wN;
    if (FAST) { float b = dn * dn; b = b * b; b = b * b; b = b * b; wN = b * b; } // det_powi(dn, 32): r = 1 * b^32
    else wN = det_pow_auto(dn, phi_n);
    const float wL = div_by(fabsf(cl - sl), phi_l);   // correctly rounded, denominator work shared by the taps of a pixel
    return det_exp((0.0f - max2(wL, 0.0f)) - max2(wZ, 0.0f)) * wN;
}

// RADIUS >= 0: compile-time filter radius (the reference default is 1: a fully unrolled 3x3 stencil with
// constant kernel weights); RADIUS < 0: run-time radius.
template <int RADIUS, bool FAST>
__global__ __launch_bounds__(256) void k_shadows_atrous(AtrousArgs a)
{
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int y = a.y0 + blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= a.w || y >= a.y1) return;
    const size_t o = (size_t)y * a.w + x;
    if (!a.tile_class[(size_t)(y >> 3) * a.tiles_x + (x >> 3)])
    {
        a.out[o] = 0u; // shadows_denoise_copy_shadow_tiles.comp:35
        if (a.out2) a.out2[o] = 0u;
        return;
    }
    const uint32_t c  = a.in.p[o];
    // RADIUS == 1: issue every load of this pixel (centre, 3x3 variance taps, decoded normals, the 8 stencil taps)
    // before the first use, so the wave pays ONE memory round trip instead of three dependent ones.
    uint32_t t_in[8];
    float4   t_nd[8];
    bool     t_ok[8];
    if (RADIUS == 1)
    {
#pragma unroll
        for (int t = 0; t < 8; t++)
        {
            const int k = t < 4 ? t : t + 1, xx = k % 3 - 1, yy = k / 3 - 1;
            const int px = x + xx * a.step, py = y + yy * a.step;
            t_ok[t] = px >= 0 && py >= 0 && px < a.w && py < a.h;
            const bool res = t_ok[t] && py >= a.y0 && py < a.y1;
            t_in[t] = res ? a.in.p[(size_t)py * a.w + px] : 0u;
            t_nd[t] = res ? a.nd[(size_t)py * a.w + px] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    const float    cv = h2f_lo(c);
    // compute_variance_center (:65-88)
    float var = 0.0f;
#pragma unroll
    for (int yy = -1; yy <= 1; yy++)
#pragma unroll
        for (int xx = -1; xx <= 1; xx++)
        {
            const float k = (xx == 0 ? (yy == 0 ? 0.25f : 0.125f) : (yy == 0 ? 0.125f : 0.0625f));
            var += h2f_hi(a.in.raw(x + xx, y + yy)) * k;
        }
    const float4 cnd = a.nd[o];
    const float center_depth = cnd.w;
    uint32_t    result;
    if (center_depth < 0.0f) result = c;
    else
    {
        const f3    cn    = mk3(cnd.x, cnd.y, cnd.z);
        const DivBy phi_v = div_prepare(a.phi_visibility * hr_sqrt(max2(0.0f, 1e-10f + var)));
        float sum_w = 1.0f, sum_v = cv, sum_var = h2f_hi(c);
        if (RADIUS == 1)
        {
            // Weights of all eight taps first, UNCONDITIONALLY (a tap outside the image was loaded as zeros: finite math,
            // weight unused) — the eight dependent exp -> divide -> exp chains then interleave instead of running one
            // after the other behind per-tap branches; measured 25.3 -> 22.8 us per iteration.  The accumulation below
            // keeps the reference's order (yy outer, xx inner) and skips the outside taps.
            float w8[8];
#pragma unroll
            for (int t = 0; t < 8; t++)
                w8[t] = edge_weight<FAST>(center_depth, t_nd[t].w, a.sigma_depth, cn, mk3(t_nd[t].x, t_nd[t].y, t_nd[t].z), a.phi_normal, cv, h2f_lo(t_in[t]), phi_v);
#pragma unroll
            for (int t = 0; t < 8; t++)
            {
                if (!t_ok[t]) continue;
                const int   k = t < 4 ? t : t + 1, xx = k % 3 - 1, yy = k / 3 - 1;
                const float kx = xx == 0 ? 1.0f : __fdiv_rn(2.0f, 3.0f), ky = yy == 0 ? 1.0f : __fdiv_rn(2.0f, 3.0f);
                const float sv = h2f_lo(t_in[t]);
                const float wv = w8[t] * (kx * ky);
                sum_w += wv;
                sum_v += wv * sv;
                sum_var += (wv * wv) * h2f_hi(t_in[t]);
            }
        }
        else
        {
        const int R = RADIUS >= 0 ? RADIUS : a.radius;
        for (int yy = -R; yy <= R; yy++)
            for (int xx = -R; xx <= R; xx++)
            {
                const int px = x + xx * a.step, py = y + yy * a.step;
                if (px < 0 || py < 0 || px >= a.w || py >= a.h || (xx == 0 && yy == 0)) continue;
                const int   axx = xx < 0 ? -xx : xx, ayy = yy < 0 ? -yy : yy;
                const float kx = axx == 0 ? 1.0f : (axx == 1 ? __fdiv_rn(2.0f, 3.0f) : __fdiv_rn(1.0f, 6.0f));
                const float ky = ayy == 0 ? 1.0f : (ayy == 1 ? __fdiv_rn(2.0f, 3.0f) : __fdiv_rn(1.0f, 6.0f));
                const uint32_t s  = a.in.raw(px, py);
                const float4   snd = (py >= a.y0 && py < a.y1) ? a.nd[(size_t)py * a.w + px] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float    sv = h2f_lo(s);
                const f3       sn = mk3(snd.x, snd.y, snd.z);
                const float    w  = edge_weight<FAST>(center_depth, snd.w, a.sigma_depth, cn, sn, a.phi_normal, cv, sv, phi_v);
                const float    wv = w * (kx * ky);
                sum_w += wv;
                sum_v += wv * sv;
                sum_var += (wv * wv) * h2f_hi(s);
            }
        }
        float ov = __fdiv_rn(sum_v, sum_w), ovar = __fdiv_rn(sum_var, sum_w * sum_w);
        if (a.power != 0.0f) ov = det_pow_auto(ov, a.power);
        result = pack_h2(ov, ovar);
    }
    a.out[o] = result;
    if (a.out2) a.out2[o] = result;
}

// ------------------------------------------------------------------------------------------------
struct hr_shadows : PassCore
{
    DevBuf  mask, temporal_out, moments[2], prev_image, atrous[2], nd, occluder;
    int     temporal_paths = TP_ALL;  // developer A/B switch HR_TEMPORAL_PAIRS=0 (pass_args.h TemporalPaths; read once at create)
    bool    occluder_cache = true;    // developer A/B switch HR_SHADOW_CACHE=0 (read once at create)
    int     read_idx = 0;             // ATrous::read_idx
    int     last_ping_pong = 0;
    int           latched_exact = -1;       // arithmetic mode of the last temporal stage: the `nd` side image it wrote has a mode-specific layout
    // developer switches (tools/timeline.py, tools/passbench.py), read from the environment ONCE in hr_shadows_create — the
    // render path never calls getenv
    int           dbg_only_tx = -1, dbg_only_ty = -1;
    bool          dbg_skip_traversal = false, dbg_skip_reproject = false, dbg_timeline_stats = false;
    std::string   dbg_timeline;             // HR_DEBUG_TIMELINE=<file>
    uint64_t      last_wave_max_steps = 0; // sum over waves of the slowest lane's (node + triangle) steps
    // tolerance mode: the geometry records (pass_core.h GeoRecords) alternate between the two halves of `nd`; the parity mode's float4 layout covers both
    void*         nd_cur = nullptr;         // the side image of the frame in flight (a-trous stages)
    // tolerance mode, fused chain: the residency cap of kf_shadows_atrous01, as bytes of unused dynamic LDS (pass_core.h atrous_resident_pad; fixed at create)
    int           atrous01_pad = 0;
    std::string   dbg_atrous_timeline;      // HR_DEBUG_ATROUS_TIMELINE=<prefix> (tools/atrous_balance.py)
};

// How many workgroups of kf_shadows_atrous01 a CU may hold (docs/EXPERIMENTS.md, "Shadow a-trous chain: live workgroups per CU", has the
// sweep: 1080p 21.9 us without, 19.8 / 19.6 / 19.3 / 20.6 at 4 / 5 / 6 / 7); 0: as many as fit (8).  HR_ATROUS01_RESIDENT, read once in
// hr_shadows_create, overrides it (A/B runs, tests).  Applied to images of at most HR_ATROUS01_REGIONS_PER_SLOT regions per slot.
#ifndef FT_ATROUS01_RESIDENT
#define FT_ATROUS01_RESIDENT 6
#endif
#ifndef HR_ATROUS01_REGIONS_PER_SLOT
#define HR_ATROUS01_REGIONS_PER_SLOT 4
#endif
#define HR_LDS_GRANULE 1280        // gfx950 allocates LDS in blocks of 320 dwords

// developer switch HR_DEBUG_ATROUS_TIMELINE=<prefix>: the per-wave records of ONE launch go to <prefix>.<tag>, rewritten by every frame
// (synchronises and allocates: never in a timed run)
struct AtrousTimelineDump
{
    DevBuf buf;
    unsigned long long* ptr() const { return (unsigned long long*)buf.p; }
    hr_status begin(const std::string& prefix, const AtrousArgs& a)
    {
        if (prefix.empty()) return HR_OK;
        return buf.alloc((size_t)shadows_atrous_max_workgroups(a) * 4 * 32);   // zeroed: a wave that wrote nothing has entry time 0
    }
    hr_status end(const std::string& prefix, const char* tag, hipStream_t st)
    {
        if (!buf.p) return HR_OK;
        HR_HIP(hipStreamSynchronize(st));
        std::vector<unsigned long long> host(buf.bytes / 8);
        HR_HIP(hipMemcpy(host.data(), buf.p, buf.bytes, hipMemcpyDeviceToHost));
        if (FILE* f = fopen((prefix + "." + tag).c_str(), "wb")) { fwrite(host.data(), 8, host.size(), f); fclose(f); }
        return HR_OK;
    }
};

bool hr::profiling_enabled(const hr_shadows* p) { return p && p->prof.enabled; }

extern "C" {

void hr_shadows_default_params(hr_shadows_params* p)
{
    p->denoise = 1; p->bias = 0.5f; p->alpha = 0.01f; p->moments_alpha = 0.2f; p->phi_visibility = 10.0f;
    p->phi_normal = 32.0f; p->sigma_depth = 1.0f; p->power = 1.2f; p->radius = 1; p->filter_iterations = 4; p->feedback_iteration = 1;
    p->exact = 1;
}

hr_status hr_shadows_create(hr_ctx* ctx, int32_t full_width, int32_t full_height, hr_scale scale, const hr_band* band, hr_shadows** out)
{
    hr_shadows* p = nullptr;
    hr_status   s = pass_new(&p, ctx, full_width, full_height, scale, band, out, BandRule::Shadows, "shadows");
    if (s != HR_OK) return s;
    if (const char* e = getenv("HR_DEBUG_ONLY_TILE")) sscanf(e, "%d,%d", &p->dbg_only_tx, &p->dbg_only_ty);
    if (const char* e = getenv("HR_SHADOW_CACHE")) p->occluder_cache = atoi(e) != 0;
    if (const char* e = getenv("HR_TEMPORAL_PAIRS")) p->temporal_paths = atoi(e) != 0 ? (p->temporal_paths | TP_PAIRS) : (p->temporal_paths & ~TP_PAIRS);
    p->tile_order.min_spread = HR_ORDER_COHERENT_SPREAD;   // rays towards one light: coherent
    p->dbg_skip_traversal = getenv("HR_DEBUG_SKIP_TRAVERSAL") != nullptr;
    p->dbg_skip_reproject = getenv("HR_DEBUG_SKIP_REPROJECT") != nullptr;
    p->dbg_timeline_stats = getenv("HR_DEBUG_TIMELINE_STATS") != nullptr;
    if (const char* e = getenv("HR_DEBUG_TIMELINE")) p->dbg_timeline = e;
    if (const char* e = getenv("HR_DEBUG_ATROUS_TIMELINE")) p->dbg_atrous_timeline = e;
    {
        int resident = FT_ATROUS01_RESIDENT;
        if (const char* e = getenv("HR_ATROUS01_RESIDENT")) resident = atoi(e);
        hipDeviceProp_t prop;
        if (resident >= 3 && hipGetDeviceProperties(&prop, ctx->device) == hipSuccess)
        {
            // The cap pays while the live workgroups of a launch (about 30 % of the regions on the bench scenes) all fit into the
            // resident * CUs slots at once; past that the live ones that wait for a slot start late and the launch is slower than without
            // (3840 x 2160: 45.5 -> 47.7 us at 6, -> 49.9 at 5).  The host knows the regions, not the live ones: a quarter of them per slot.
            const int own = shadows_atrous01_static_lds(), regions = cdiv(p->w, 32) * cdiv(p->y1 - p->y0, 16);
            if (regions > HR_ATROUS01_REGIONS_PER_SLOT * resident * prop.multiProcessorCount) resident = 0;
            if (own >= 0) p->atrous01_pad = atrous_resident_pad((int)prop.maxSharedMemoryPerMultiProcessor, own, resident, HR_LDS_GRANULE);
            if (own + p->atrous01_pad > (int)prop.sharedMemPerBlock) p->atrous01_pad = 0;   // more than a workgroup may ask for: no cap
        }
    }
    const size_t px = (size_t)p->w * p->h; // full-frame sized (bands index with absolute rows)
    HR_PASS_ALLOC(mask, (size_t)p->mw * p->mh * 4)
    HR_PASS_ALLOC(temporal_out, px * 4)
    HR_PASS_ALLOC(moments[0], px * 8)
    HR_PASS_ALLOC(moments[1], px * 8)
    HR_PASS_ALLOC(prev_image, px * 4)
    HR_PASS_ALLOC(atrous[0], px * 4)
    HR_PASS_ALLOC(atrous[1], px * 4)
    HR_PASS_ALLOC(upsample, (size_t)full_width * full_height * 2)
    // + 8 readable bytes: kf_shadows_atrous fetches the classes of a workgroup's four tiles as the two aligned dwords that hold them
    HR_PASS_ALLOC(tile_class, (((size_t)p->tiles_x * p->tiles_y + 3) & ~(size_t)3) + 8)
    HR_PASS_ALLOC(nd, px * 16)
    HR_PASS_ALLOC(counters, 64)
    HR_PASS_ALLOC(ray_slots, (size_t)p->tiles_x * p->tiles_y * 2)
    HR_PASS_ALLOC(occluder, px * 4)
    if ((s = p->tile_order.init(p->resident_tiles())) != HR_OK) { delete p; return s; }
    HR_HIP(hipMemset(p->occluder.p, 0xff, p->occluder.bytes));   // no cached occluder
    HR_HIP(hipMemset(p->counters.p, 0, 64));
    HR_HIP(hipMemset(p->ray_slots.p, 0, p->ray_slots.bytes));
    HR_HIP(hipMemset(p->mask.p, 0, p->mask.bytes));
    HR_HIP(hipMemset(p->tile_class.p, 0, p->tile_class.bytes));
    *out = p;
    return HR_OK;
}

hr_status hr_shadows_destroy(hr_shadows* p) { return pass_destroy(p); }
hr_status hr_shadows_reset_history(hr_shadows* p) { return pass_reset_history(p); }
hr_status hr_shadows_history_apron_exceeded(hr_shadows* p, int32_t* exceeded) { return pass_history_apron_exceeded(p, exceeded); }
hr_status hr_shadows_set_profiling(hr_shadows* p, int32_t enable) { return pass_set_profiling(p, enable); }
hr_status hr_shadows_get_stage_times(hr_shadows* p, hr_stage_times* out) { return pass_get_stage_times(p, out); }
hr_status hr_shadows_ray_count(hr_shadows* p, uint64_t* rays) { return pass_ray_count<uint16_t>(p, rays); }
hr_status hr_shadows_launch_order(hr_shadows* p, uint32_t* out, int32_t* n_tiles) { return pass_launch_order(p, out, n_tiles); }

hr_status hr_shadows_tile_ray_counts(hr_shadows* p, uint16_t* out, int32_t* tiles_x, int32_t* tiles_y)
{
    HR_CHECK_ARG(p);
    if (tiles_x) *tiles_x = p->tiles_x;
    if (tiles_y) *tiles_y = p->tiles_y;
    if (!out) return HR_OK;
    HR_HIP(hipStreamSynchronize(p->last_stream));
    HR_HIP(hipMemcpy(out, p->ray_slots.p, (size_t)p->tiles_x * p->tiles_y * 2, hipMemcpyDeviceToHost));
    return HR_OK;
}

hr_status hr_shadows_ray_trace(hr_shadows* p, const hr_scene* scene, const hr_frame_inputs* in, const hr_shadows_params* prm, void* stream_)
{
    HR_CHECK_ARG(p && scene && in && prm);
    hr_status s = check_inputs(p, in, false);
    if (s != HR_OK) return s;
    HR_CHECK_ARG(in->sobol && in->scrambling_ranking);
    // statistics, timelines and the debug switches
    HR_REJECT_SHARED_DEV(scene, "hr_shadows_ray_trace", p->want_stats || !p->dbg_timeline.empty() || p->dbg_skip_traversal || p->dbg_only_tx >= 0);
    HR_REJECT_CUTOUT(scene, HR_RAY_SHADOW, "hr_shadows_ray_trace", p->want_stats || !p->dbg_timeline.empty() || p->dbg_skip_traversal || p->dbg_only_tx >= 0);
    const bool       cutout = cutout_on(scene, HR_RAY_SHADOW);
    const CutoutView cv = cutout ? cutout_view_of(scene) : CutoutView();
    hipStream_t st = (hipStream_t)stream_;
    p->last_stream = st;
    // clear_images() (ray_traced_shadows.cpp:938-968): first frame zeroes the feedback image and the
    // history moments slot that will be read.
    if (p->first_frame)
    {
        HR_HIP(hipMemsetAsync(p->prev_image.p, 0, p->prev_image.bytes, st));
        HR_HIP(hipMemsetAsync(p->moments[!in->ping_pong].p, 0, p->moments[0].bytes, st));
        p->first_frame = false;
    }
    TraceArgs a;
    for (int i = 0; i < 16; i++) a.vpi[i] = in->ubo.view_proj_inverse[i];
    a.light = in->ubo.light;
    a.depth = in->cur.depth; a.gb2 = (const uint2*)in->cur.gb2;
    a.sobol = in->sobol; a.sr = in->scrambling_ranking;
    a.mask = (uint32_t*)p->mask.p; a.ray_slots = (uint16_t*)p->ray_slots.p;
    a.nodes = (const Node8*)scene->nodes.p; a.tris = (const TriGPU*)scene->tris.p; a.inst = (const InstanceShared*)scene->inst_shared.p; a.cull = cull_of(scene, HR_RAY_SHADOW);
    a.stats = nullptr;
    a.timeline = nullptr;
    a.w = p->w; a.h = p->h; a.y0 = p->y0; a.y1 = p->y1; a.mw = p->mw;
    a.tile_y0 = p->tile_y0(); a.tiles_x = p->tiles_x; a.tiles_y = p->resident_tiles_y();
    a.bias = prm->bias; a.num_frames = in->num_frames;
    a.occluder = p->occluder_cache ? (uint32_t*)p->occluder.p : nullptr;
    a.n_tri_refs = (uint32_t)(scene->tris.bytes / sizeof(TriGPU));
    const int n_tiles = a.tiles_x * a.tiles_y;
    const int n_slots = n_tiles;
    a.debug_only_tx = p->dbg_only_tx; a.debug_only_ty = p->dbg_only_ty;
    a.debug_skip_traversal = p->dbg_skip_traversal ? 1 : 0;
    if ((s = p->tile_order.flush(st)) != HR_OK) return s;   // last launch's costs, if no temporal stage took them along
    a.order = p->tile_order.order_arg(n_tiles); a.cost = p->tile_order.cost_arg(n_tiles);
    const uint64_t px = (uint64_t)p->w * (p->y1 - p->y0);
    if (p->want_stats)
    {
        a.cost = nullptr;
        // instrumented build of the same kernel: counts node visits / triangle tests
        HR_HIP(hipMemsetAsync((char*)p->counters.p + 16, 0, 24, st));
        a.stats = (unsigned long long*)((char*)p->counters.p + 16);
        hipLaunchKernelGGL(k_shadows_trace<true>, dim3(cdiv(n_slots, TRACE_WAVES)), dim3(64 * TRACE_WAVES), 0, st, a, cv);
        HR_HIP(hipGetLastError());
        return HR_OK;
    }
    if (!p->dbg_timeline.empty())
    {
        const char* tl = p->dbg_timeline.c_str();
        // developer switch (tools/timeline.py): per-wave start/end ticks of ONE launch of the tile kernel, written to the file
        DevBuf buf;
        hr_status bs = buf.alloc((size_t)n_tiles * 32);
        if (bs != HR_OK) return bs;
        a.timeline = (unsigned long long*)buf.p;
        if (p->dbg_timeline_stats) hipLaunchKernelGGL(k_shadows_trace<true>, dim3(cdiv(n_slots, TRACE_WAVES)), dim3(64 * TRACE_WAVES), 0, st, a, cv);
        else hipLaunchKernelGGL(k_shadows_trace<false>, dim3(cdiv(n_slots, TRACE_WAVES)), dim3(64 * TRACE_WAVES), 0, st, a, cv);
        HR_HIP(hipStreamSynchronize(st));
        std::vector<unsigned long long> host((size_t)n_tiles * 4);
        HR_HIP(hipMemcpy(host.data(), buf.p, host.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = fopen(tl, "wb")) { fwrite(host.data(), 8, host.size(), f); fclose(f); }
        a.timeline = nullptr;
    }
    int ev = p->prof.begin("ray_trace", st, px * 12 + px / 8);
    // a shared scene arrives here too: HR_REJECT_SHARED_DEV has refused everything above for it
    const auto kernel = scene->shared ? (cutout ? k_shadows_trace<false, true, true> : k_shadows_trace<false, true>)
                                      : (cutout ? k_shadows_trace<false, false, true> : k_shadows_trace<false>);
    hipLaunchKernelGGL(kernel, dim3(cdiv(n_slots, TRACE_WAVES)), dim3(64 * TRACE_WAVES), 0, st, a, cv);
    p->prof.end(ev, st);
    HR_HIP(hipGetLastError());
    if (a.cost && (s = p->tile_order.traced(n_tiles, st)) != HR_OK) return s;
    return HR_OK;
}

hr_status hr_shadows_trace_divergence(hr_shadows* p, uint64_t* wave_max_steps)
{
    HR_CHECK_ARG(p && wave_max_steps);
    *wave_max_steps = p->last_wave_max_steps;
    return HR_OK;
}

static hr_status shadows_trace_stats_impl(hr_shadows* p, const hr_scene* scene, const hr_frame_inputs* in, const hr_shadows_params* prm, uint64_t* out3, void* stream, bool walk_only)
{
    HR_CHECK_ARG(p && out3);
    // walk_only: the counts are those of the WALK (SURVEY 8d's BVH term, comparable between frames and builds): the occluder cache, whose
    // contents depend on the previous frames, is bypassed for the statistics pass.  Otherwise: the counts of the kernel render() launches
    const bool cache = p->occluder_cache;
    p->want_stats = true;
    if (walk_only) p->occluder_cache = false;
    hr_status s = hr_shadows_ray_trace(p, scene, in, prm, stream);
    p->want_stats = false;
    p->occluder_cache = cache;
    if (s != HR_OK) return s;
    HR_HIP(hipStreamSynchronize((hipStream_t)stream));
    uint64_t host[5];
    HR_HIP(hipMemcpy(host, p->counters.p, 40, hipMemcpyDeviceToHost));
    hr_status rs = hr_shadows_ray_count(p, &out3[0]);
    if (rs != HR_OK) return rs;
    out3[1] = host[2]; out3[2] = host[3];
    p->last_wave_max_steps = host[4];
    return HR_OK;
}

hr_status hr_shadows_trace_stats(hr_shadows* p, const hr_scene* scene, const hr_frame_inputs* in, const hr_shadows_params* prm, uint64_t* out3, void* stream)
{
    return shadows_trace_stats_impl(p, scene, in, prm, out3, stream, true);
}

hr_status hr_shadows_trace_stats_timed(hr_shadows* p, const hr_scene* scene, const hr_frame_inputs* in, const hr_shadows_params* prm, uint64_t* out3, void* stream)
{
    return shadows_trace_stats_impl(p, scene, in, prm, out3, stream, false);
}

hr_status hr_shadows_temporal(hr_shadows* p, const hr_frame_inputs* in, const hr_shadows_params* prm, void* stream_)
{
    HR_CHECK_ARG(p && in && prm);
    hr_status s = check_inputs(p, in, true);
    if (s != HR_OK) return s;
    hipStream_t st = (hipStream_t)stream_;
    p->last_stream = st;
    p->latched_exact = prm->exact ? 1 : 0;
    TemporalArgs a;
    for (int i = 0; i < 16; i++) a.vpi[i] = in->ubo.view_proj_inverse[i];
    a.mask = (const uint32_t*)p->mask.p; a.mw = p->mw; a.mh = p->mh;
    const int w = p->w, y0 = p->y0, y1 = p->y1, ry0 = p->ry0, ry1 = p->ry1;
    a.gb2  = ImgRGBA16F { (const uint2*)in->cur.gb2, w, ry0, ry1 };
    a.gb3  = ImgRGBA16F { (const uint2*)in->cur.gb3, w, ry0, ry1 };
    a.pgb2 = ImgRGBA16F { (const uint2*)in->prev.gb2, w, ry0, ry1 };
    a.pgb3 = ImgRGBA16F { (const uint2*)in->prev.gb3, w, ry0, ry1 };
    a.depth  = ImgR32F { in->cur.depth, w, ry0, ry1 };
    a.pdepth = ImgR32F { in->prev.depth, w, ry0, ry1 };
    a.hist         = ImgRG16F { (const uint32_t*)p->prev_image.p, w, ry0, ry1 };
    a.hist_moments = ImgRGBA16F { (const uint2*)p->moments[!in->ping_pong].p, w, ry0, ry1 };
    a.out = (uint32_t*)p->temporal_out.p; a.out_moments = (uint2*)p->moments[in->ping_pong ? 1 : 0].p;
    a.tile_class = (uint8_t*)p->tile_class.p;
    a.nd = (float4*)p->nd.p;
    a.geo_hist = nullptr;
    a.apron = GeoApronArgs { nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, -1 };
    if (!prm->exact)
    {
        // the records of the last frame stand for in->prev when the caller hands back what it passed as in->cur then; a band keeps to
        // the caller's images (its records cover the rows it computed, not the history apron its neighbours own)
        // (round 5: bands too — the records of the rows a band reads history from but does not compute, hr_band.history_halo beyond
        // hr_band.halo, are copies of the current G-buffer as well, written by a few extra workgroups of the temporal launch: GeoApronArgs)
        const size_t half = (size_t)p->w * p->h * 8;
        const GeoRecords::Step g = p->records.advance(in->cur.gb2, in->cur.gb3, in->prev.gb2, in->prev.gb3, p->first_frame);
        if (g.read >= 0) a.geo_hist = (const char*)p->nd.p + (size_t)g.read * half;
        a.nd = (float4*)((char*)p->nd.p + (size_t)g.write * half);
        if (p->records.history && (ry0 < y0 || ry1 > y1))
            a.apron = GeoApronArgs { in->cur.gb2, in->cur.gb3, a.nd, w, ry0, y0, y1, ry1, -1 };
        if (g.require_failed) return geo_require_error("hr_shadows_temporal");
    }
    else p->records.invalidate();   // the parity mode's float4 layout covers both halves
    p->nd_cur = a.nd;
    a.w = w; a.h = p->h; a.y0 = y0; a.y1 = y1;
    a.tile_y0 = p->tile_y0(); a.tiles_x = p->tiles_x; a.tiles_y = p->resident_tiles_y();
    a.alpha = prm->alpha; a.moments_alpha = prm->moments_alpha;
    a.debug_skip_reproject = p->dbg_skip_reproject ? 1 : 0;
    a.apron_flag = p->apron_flag();
    a.band_y0 = p->band_y0; a.band_y1 = p->band_y1;
    a.paths = p->temporal_paths;
    p->last_ping_pong = in->ping_pong ? 1 : 0;
    const uint64_t px = (uint64_t)w * (y1 - y0);
    int ev = p->prof.begin("temporal_accumulation", st, px * 64 + px / 8);
    a.sort = TileSortArgs { nullptr, nullptr, 0, 0, 0, 0 };
    if (prm->exact) hipLaunchKernelGGL(k_shadows_temporal, dim3(cdiv(a.tiles_x * a.tiles_y, TEMPORAL_WAVES)), dim3(64 * TEMPORAL_WAVES), 0, st, a);
    else
    {
        a.sort = p->tile_order.ride();   // the trace kernel's next launch order rides along (tile_order.h)
        launch_shadows_temporal_fast(a, a.tiles_x * a.tiles_y, st);
    }
    p->prof.end(ev, st);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

static hr_status check_mode(hr_shadows* p, const hr_shadows_params* prm);

hr_status hr_shadows_atrous_iteration(hr_shadows* p, const hr_frame_inputs* in, const hr_shadows_params* prm, int32_t i, void* stream_)
{
    HR_CHECK_ARG(p && in && prm && i >= 0 && i < prm->filter_iterations && prm->filter_iterations <= 8 && prm->radius >= 0 && prm->radius <= 2);
    hr_status s = check_inputs(p, in, false);
    if (s != HR_OK) return s;
    if ((s = check_mode(p, prm)) != HR_OK) return s;
    hipStream_t st = (hipStream_t)stream_;
    p->last_stream = st;
    // ping-pong as a_trous_filter() (:1101-1107,1175): read = i odd, write = i even ? 1 : 0
    const int read_idx = i & 1, write_idx = (i & 1) ^ 1;
    AtrousArgs a;
    const int w = p->w, y0 = p->y0, y1 = p->y1;
    a.in  = ImgRG16F { (const uint32_t*)(i == 0 ? p->temporal_out.p : p->atrous[read_idx].p), w, y0, y1 };
    a.nd = (const float4*)(p->nd_cur ? p->nd_cur : p->nd.p);
    a.tile_class = (const uint8_t*)p->tile_class.p;
    a.out  = (uint32_t*)p->atrous[write_idx].p;
    a.out2 = (prm->feedback_iteration == i) ? (uint32_t*)p->prev_image.p : nullptr; // vkCmdCopyImage :1177-1207
    a.w = w; a.h = p->h; a.y0 = y0; a.y1 = y1; a.tiles_x = p->tiles_x;
    a.radius = prm->radius; a.step = 1 << i;
    a.phi_visibility = prm->phi_visibility; a.phi_normal = prm->phi_normal; a.sigma_depth = prm->sigma_depth;
    a.power = (i == prm->filter_iterations - 1) ? prm->power : 0.0f;
    p->read_idx = write_idx;
    static const char* names[8] = { "atrous_0", "atrous_1", "atrous_2", "atrous_3", "atrous_4", "atrous_5", "atrous_6", "atrous_7" };
    const uint64_t px = (uint64_t)w * (y1 - y0);
    int ev = p->prof.begin(names[i], st, px * 24 + (a.out2 ? px * 4 : 0));
    const dim3 grid(cdiv(w, 32), cdiv(y1 - y0, 8));
    const bool fast = (prm->phi_normal == 32.0f && prm->sigma_depth == 1.0f);
    AtrousTimelineDump tl;   // developer switch HR_DEBUG_ATROUS_TIMELINE: iterations 2 and 3 of the fused chain
    if (!prm->exact && p->fuse && prm->radius == 1 && (i == 2 || i == 3) && (s = tl.begin(p->dbg_atrous_timeline, a)) != HR_OK) return s;
    if (!prm->exact) launch_shadows_atrous_fast(a, st, tl.ptr());
    else if (prm->radius == 1 && fast) hipLaunchKernelGGL((k_shadows_atrous<1, true>), grid, dim3(256), 0, st, a);
    else if (prm->radius == 1) hipLaunchKernelGGL((k_shadows_atrous<1, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_shadows_atrous<-1, false>), grid, dim3(256), 0, st, a);
    p->prof.end(ev, st);
    HR_HIP(hipGetLastError());
    if ((s = tl.end(p->dbg_atrous_timeline, i == 2 ? "atrous4" : "atrous8", st)) != HR_OK) return s;
    return HR_OK;
}

// the temporal stage writes the normal / depth side image `nd` in a mode-specific layout (packed uint2 in tolerance mode, float4 in the
// parity mode): an a-trous stage in the other mode would read garbage — refuse it instead (round-2 advisor)
static hr_status check_mode(hr_shadows* p, const hr_shadows_params* prm)
{
    if (p->latched_exact >= 0 && p->latched_exact != (prm->exact ? 1 : 0))
    {
        set_last_error("hr_shadows: params.exact changed between the temporal and the a-trous stage of one frame");
        return HR_ERR_INVALID_ARG;
    }
    return HR_OK;
}

// tolerance mode, radius 1: iterations 0 and 1 in one launch (kf_shadows_atrous01; iteration 0's image stays in LDS)
static hr_status shadows_atrous01(hr_shadows* p, const hr_frame_inputs* in, const hr_shadows_params* prm, void* stream_, bool* done)
{
    hr_status s = check_inputs(p, in, false);
    if (s != HR_OK) return s;
    if ((s = check_mode(p, prm)) != HR_OK) return s;
    hipStream_t st = (hipStream_t)stream_;
    p->last_stream = st;
    AtrousArgs a;
    const int w = p->w, y0 = p->y0, y1 = p->y1;
    a.in  = ImgRG16F { (const uint32_t*)p->temporal_out.p, w, y0, y1 };
    a.nd = (const float4*)(p->nd_cur ? p->nd_cur : p->nd.p);
    a.tile_class = (const uint8_t*)p->tile_class.p;
    a.out  = (uint32_t*)p->atrous[0].p;   // iteration 1 writes atrous[0] (ping-pong of a_trous_filter(), :1101-1107)
    a.out2 = (prm->feedback_iteration == 1) ? (uint32_t*)p->prev_image.p : nullptr;
    uint32_t* first2 = (prm->feedback_iteration == 0) ? (uint32_t*)p->prev_image.p : nullptr;
    a.w = w; a.h = p->h; a.y0 = y0; a.y1 = y1; a.tiles_x = p->tiles_x;
    a.radius = prm->radius; a.step = 1;
    a.phi_visibility = prm->phi_visibility; a.phi_normal = prm->phi_normal; a.sigma_depth = prm->sigma_depth;
    a.power = 0.0f;
    const uint64_t px = (uint64_t)w * (y1 - y0);
    // algorithmic bytes: in 4 + normal/depth 8 + out 4 (+ 4 feedback); the G-buffer side image counts once
    AtrousTimelineDump tl;
    if ((s = tl.begin(p->dbg_atrous_timeline, a)) != HR_OK) return s;
    int ev = p->prof.begin("atrous_01", st, px * 16 + ((a.out2 || first2) ? px * 4 : 0));
    *done = launch_shadows_atrous01_fast(a, first2, prm->filter_iterations == 2 ? prm->power : 0.0f, st, p->atrous01_pad, tl.ptr());
    p->prof.end(ev, st);
    if ((s = tl.end(p->dbg_atrous_timeline, "atrous01", st)) != HR_OK) return s;
    if (*done) p->read_idx = 0;
    HR_HIP(hipGetLastError());
    return HR_OK;
}

hr_status hr_shadows_upsample(hr_shadows* p, const hr_frame_inputs* in, const hr_shadows_params* prm, void* stream)
{
    HR_CHECK_ARG(p && in && prm);
    const uint64_t PX = (uint64_t)p->full_w * p->full_h, px = (uint64_t)p->w * p->h;
    return pass_upsample(p, in, prm->exact != 0, p->atrous[p->read_idx].p, 2, 1, 0.0f, 0.0f, PX * 18 + px * 20, stream);
}

// Everything of RayTracedShadows::render after the ray trace (ray_traced_shadows.cpp:104-113): temporal accumulation, the a-trous
// chain, the upsample of a scaled pass.  A caller that overlaps work with the trace (row bands: the history exchange) calls
// hr_shadows_ray_trace + hr_shadows_denoise instead of hr_shadows_render and gets the same launches — in tolerance mode the fused ones.
hr_status hr_shadows_denoise(hr_shadows* p, const hr_frame_inputs* in, const hr_shadows_params* prm, void* stream)
{
    HR_CHECK_ARG(p && in && prm);
    p->last_denoise = prm->denoise != 0;
    if (!prm->denoise) return HR_OK;
    hr_status s;
    if ((s = hr_shadows_temporal(p, in, prm, stream)) != HR_OK) return s;
    {
        HR_SCOPED_SAMPLE("A-Trous Filter");   // ray_traced_shadows.cpp:1096
        bool fused = false;
        if (!prm->exact && p->fuse && prm->filter_iterations >= 2 && prm->filter_iterations <= 8 && prm->radius == 1 &&
            (s = shadows_atrous01(p, in, prm, stream, &fused)) != HR_OK) return s;
        for (int i = fused ? 2 : 0; i < prm->filter_iterations; i++)
            if ((s = hr_shadows_atrous_iteration(p, in, prm, i, stream)) != HR_OK) return s;
    }
    if (p->scale != 0 && (s = hr_shadows_upsample(p, in, prm, stream)) != HR_OK) return s;
    return HR_OK;
}

hr_status hr_shadows_render(hr_shadows* p, const hr_scene* scene, const hr_frame_inputs* in, const hr_shadows_params* prm, void* stream)
{
    HR_SCOPED_SAMPLE("Ray Traced Shadows");
    HR_CHECK_ARG(p && scene && in && prm);
    HR_HIP(hipSetDevice(p->ctx->device));
    p->prof.begin_frame();
    p->last_denoise = prm->denoise != 0;
    hr_status s = hr_shadows_ray_trace(p, scene, in, prm, stream);
    if (s != HR_OK) return s;
    return hr_shadows_denoise(p, in, prm, stream);
}

hr_status hr_shadows_image(hr_shadows* p, int32_t which, hr_image_view* v)
{
    HR_CHECK_ARG(p && v);
    switch (which)
    {
        case 0: fill_view(v, p->mask.p, p->mw, p->mh, 4, HR_FORMAT_R32_UINT); break;
        case 1: fill_view(v, p->temporal_out.p, p->w, p->h, 4, HR_FORMAT_RG16F); break;
        case 2: fill_view(v, p->moments[0].p, p->w, p->h, 8, HR_FORMAT_RGBA16F); break;
        case 3: fill_view(v, p->moments[1].p, p->w, p->h, 8, HR_FORMAT_RGBA16F); break;
        case 4: fill_view(v, p->prev_image.p, p->w, p->h, 4, HR_FORMAT_RG16F); break;
        case 5: fill_view(v, p->atrous[0].p, p->w, p->h, 4, HR_FORMAT_RG16F); break;
        case 6: fill_view(v, p->atrous[1].p, p->w, p->h, 4, HR_FORMAT_RG16F); break;
        case 7: fill_view(v, p->upsample.p, p->full_w, p->full_h, 2, HR_FORMAT_R16F); break;
        case 8: fill_view(v, p->tile_class.p, p->tiles_x, p->tiles_y, 1, (hr_format)0); break;
        case 9:   // tolerance mode: the geometry records {GB2.x, GB3.y} the last temporal stage wrote — tests / tools
            if (!p->nd_cur || p->latched_exact != 0) { set_last_error("hr_shadows_image(9): no geometry records (parity mode, or no temporal stage yet)"); return HR_ERR_INVALID_ARG; }
            fill_view(v, p->nd_cur, p->w, p->h, 8, HR_FORMAT_RGBA16F); break;
        default: set_last_error("hr_shadows_image: unknown image index"); return HR_ERR_INVALID_ARG;
    }
    return HR_OK;
}

// RayTracedShadows::output_ds (ray_traced_shadows.cpp:135-155)
hr_status hr_shadows_output(hr_shadows* p, hr_output_kind kind, hr_image_view* v)
{
    HR_CHECK_ARG(p && v);
    if (!p->last_denoise || kind == HR_OUTPUT_RAY_TRACE) return hr_shadows_image(p, 0, v);
    if (kind == HR_OUTPUT_TEMPORAL_ACCUMULATION) return hr_shadows_image(p, 1, v);
    if (kind == HR_OUTPUT_ATROUS || p->scale == 0) return hr_shadows_image(p, 5 + p->read_idx, v);
    return hr_shadows_image(p, 7, v);
}

} // extern "C"
