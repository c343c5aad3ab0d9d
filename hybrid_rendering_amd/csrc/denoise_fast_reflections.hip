// Tolerance-mode reflections denoiser: the temporal kernel and the a-trous chain (denoise_fast_common.h has what the passes share).
#include "denoise_fast_common.h"
#include "tile_order.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// reflections_denoise_reprojection.comp, tolerance mode.  32x8 tile per workgroup; the 48x24 input colours around it are staged
// in LDS as they are (fp16), and the 17x17 neighbourhood mean / standard deviation (:133-157 — 289 taps per pixel in the
// reference) become SEPARABLE sums: a horizontal pass (each thread forms four adjacent 17-tap row sums from one 20-texel window,
// sharing the 14-texel core) into LDS, then 17 row sums per pixel.
#define FR_TW 32
#define FR_TH 8
#define FR_R 8
#ifndef FR_EU
#define FR_EU 5        // minimum waves per SIMD the register allocator leaves room for (see FR_ALIAS)
#endif
#ifndef FR_ALIAS
#define FR_ALIAS 0     // 1: the horizontal sums overwrite the colour tile (the sums are held in registers across a barrier): 27.6 -> 18.4 KB of
                       // LDS per workgroup, 5 -> 8 workgroups per CU if the registers allow (FR_EU)
#endif
template <int GEO>
__global__ __launch_bounds__(256, FR_EU) void kf_refl_temporal(ReflTemporalArgs a)
{
    if (tile_order_rides<256>(a.sort)) return;   // the trace kernel's next launch order, as extra grid rows (tile_order.h)
    const uint2 BLK = block_xy<0>();
    constexpr int CW = FR_TW + 2 * FR_R, CH = FR_TH + 2 * FR_R;   // 48 x 24
#if FR_ALIAS
    __shared__ float4 s_raw[CH * FR_TW + CH * FR_TW / 2];          // 18.4 KB: first the colour tile (9.2 KB), then ha | hb
    uint2  (*s_col)[CW]   = reinterpret_cast<uint2 (*)[CW]>(s_raw);
    float4 (*s_ha)[FR_TW] = reinterpret_cast<float4 (*)[FR_TW]>(s_raw);
    float2 (*s_hb)[FR_TW] = reinterpret_cast<float2 (*)[FR_TW]>(s_raw + CH * FR_TW);
#else
    __shared__ uint2  s_col[CH][CW];        // rgb + ray length, fp16 as stored by the trace
    __shared__ float4 s_ha[CH][FR_TW];      // horizontal sums: sum r, g, b, sum r^2
    __shared__ float2 s_hb[CH][FR_TW];      //                  sum g^2, b^2
#endif
    __shared__ int    s_flag[4];
    const int bx0 = BLK.x * FR_TW, by0 = a.y0 + BLK.y * FR_TH;
    if (bx0 >= a.w) return;   // a padding column of the launch (block_map.h grid_cols)
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int x = bx0 + lx, y = by0 + ly;
    const bool have = x < a.w && y < a.y1;
    // memory round trips in this order: (1) centre texels + the 48x24 colour tile, under which nothing else can run; (2) the history
    // taps, issued after the horizontal LDS pass and left in flight under the vertical one
    const uint32_t o = have ? (uint32_t)(y * a.w + x) : (uint32_t)(a.y0 * a.w);
    const float d   = fm::ld<float>(a.depth.p, o * 4u);
    const uint2 cg2 = fm::ld<uint2>(a.gb2.p, o * 8u), cg3 = fm::ld<uint2>(a.gb3.p, o * 8u);
    if (threadIdx.x < 4) s_flag[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < CH * CW; i += 256)
    {
        const int cy = i / CW, cx = i - cy * CW;
        s_col[cy][cx] = a.in.raw(bx0 - FR_R + cx, by0 - FR_R + cy);
    }
    __syncthreads();
#if FR_ALIAS
    const uint2 cq = s_col[(threadIdx.x >> 5) + FR_R][(threadIdx.x & 31) + FR_R];   // the centre texel, before the tile is overwritten
    float4 ha_out[4];
    float2 hb_out[4];
#endif
    if (threadIdx.x < CH * (FR_TW / 4))
    {
        const int r = threadIdx.x >> 3, g = (threadIdx.x & 7) * 4;   // row, first of four adjacent outputs
        float c1[3] = { 0, 0, 0 }, c2[3] = { 0, 0, 0 };              // core: texels g+3 .. g+16, in every one of the four windows
        f3    e[6];                                                  // edge texels g+0, g+1, g+2, g+17, g+18, g+19
#pragma unroll
        for (int t = 0; t < 20; t++)
        {
            const uint2 q = s_col[r][g + t];
            const f3    c = mk3(fm::lo(q.x), fm::hi(q.x), fm::lo(q.y));
            if (t >= 3 && t <= 16)
            {
                c1[0] += c.x; c1[1] += c.y; c1[2] += c.z;
                c2[0] += c.x * c.x; c2[1] += c.y * c.y; c2[2] += c.z * c.z;
            }
            else e[t < 3 ? t : t - 14] = c;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            // window j = texels g+j .. g+j+16 = core + edge texels {j, .., 2} + {3, .., 2+j}
            float s1[3] = { c1[0], c1[1], c1[2] }, s2[3] = { c2[0], c2[1], c2[2] };
#pragma unroll
            for (int k = 0; k < 6; k++)
                if ((k < 3 && k >= j) || (k >= 3 && k - 3 < j))
                {
                    s1[0] += e[k].x; s1[1] += e[k].y; s1[2] += e[k].z;
                    s2[0] += e[k].x * e[k].x; s2[1] += e[k].y * e[k].y; s2[2] += e[k].z * e[k].z;
                }
#if FR_ALIAS
            ha_out[j] = make_float4(s1[0], s1[1], s1[2], s2[0]);
            hb_out[j] = make_float2(s2[1], s2[2]);
#else
            s_ha[r][g + j] = make_float4(s1[0], s1[1], s1[2], s2[0]);
            s_hb[r][g + j] = make_float2(s2[1], s2[2]);
#endif
        }
    }
#if FR_ALIAS
    __syncthreads();   // every thread has read its part of the colour tile
    if (threadIdx.x < CH * (FR_TW / 4))
    {
        const int r = threadIdx.x >> 3, g = (threadIdx.x & 7) * 4;
#pragma unroll
        for (int j = 0; j < 4; j++) { s_ha[r][g + j] = ha_out[j]; s_hb[r][g + j] = hb_out[j]; }
    }
#endif
    __syncthreads();
    const bool  live = have && d != 1.0f;
#if !FR_ALIAS
    const uint2 cq = s_col[ly + FR_R][lx + FR_R];
#endif
    // The pixel's program from the history taps on.  It runs once; a wave in which some history tap sat on a knife edge of the validity test (Reproj::tap_valid notes
    // it) runs it a SECOND time — a cold copy, as in kf_shadows_temporal / kf_ao_temporal — in which the noted taps take the parity kernels' verdicts
    // (Reproj::exact_bits), and stores again (late round 6: tools/fuzz_tolerance.py 6361 #385 had ONE such tap flip a pixel's moments by 92 fp16 ulp, and five a-trous
    // iterations of radius 2 spread that beyond the chain's counted allowance; docs/EXPERIMENTS.md R6.14).  The separable sums are still in LDS for it.
    bool flag = false;
    auto pixel = [&](const bool redo) -> uint32_t {
    Reproj<8, true, true, GEO> rp;
    rp.M = a.vpi; rp.pgb2 = a.pgb2.p; rp.pgb3 = a.pgb3.p; rp.pdepth = a.pdepth.p; rp.hist = a.hist.p; rp.hist_moments = a.hist_moments.p; rp.hist_len = nullptr;
    rp.geo = a.geo_hist;
    rp.g = HistGeom { a.w, a.h, a.pgb2.y0, a.pgb2.y1 };
    uint32_t ovr = 0u, known = 0u;
    if (redo && live)
    {
        rp.issue(x, y, d, cg2.y, fm::lo(cg3.y), fm::hi(cg3.x), fm::oct_unit(cg2.x), mk3(a.cam[0], a.cam[1], a.cam[2]), a.pvp, fm::hi(cq.y));
        ReprojOut r0;
        rp.template resolve<true>(r0);
        if (rp.near13)
        {
            known = rp.near13;
            ovr   = rp.exact_bits(known, x, y, d, cg2.x, cg2.y);
            if ((((ovr ^ rp.valid13) & known) & 0xfu) != 0u)   // a bilinear verdict flipped: the 3x3 fallback may run where it did not (or the other way round)
            {
                const uint32_t rest = 0x1ff0u & ~known;
                ovr |= rp.exact_bits(rest, x, y, d, cg2.x, cg2.y);
                known |= rest;
            }
        }
    }
    if (live) rp.issue(x, y, d, cg2.y, fm::lo(cg3.y), fm::hi(cg3.x), fm::oct_unit(cg2.x), mk3(a.cam[0], a.cam[1], a.cam[2]), a.pvp, fm::hi(cq.y));
    if (!redo && a.apron_flag && live && y >= a.band_y0 && y < a.band_y1 && rp.apron_miss) atomicOr(a.apron_flag, 1u);   // rare
    rp.near13 = 0u;
    // vertical pass of the separable sums (LDS only) while the history taps are in flight
    float s1[3] = { 0, 0, 0 }, s2[3] = { 0, 0, 0 };
#pragma unroll 6   // in groups: fully unrolled, the 34 LDS reads are hoisted together and cost 100 VGPRs next to the 25 tap registers
    for (int dy = 0; dy <= 2 * FR_R; dy++)
    {
        const float4 ha = s_ha[ly + dy][lx];
        const float2 hb = s_hb[ly + dy][lx];
        s1[0] += ha.x; s1[1] += ha.y; s1[2] += ha.z; s2[0] += ha.w; s2[1] += hb.x; s2[2] += hb.y;
    }
    if (have)
    {
        const float roughness = fm::lo(cg3.x);
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f, m0 = 0.0f, m1 = 0.0f, hl = 0.0f;
        if (live)
        {
            const f3  color = mk3(fm::lo(cq.x), fm::hi(cq.x), fm::lo(cq.y));
            ReprojOut r;
            const bool success = rp.template resolve<true>(r, ovr, known);
            hl = fm::fmin_(32.0f, success ? r.length + 1.0f : 1.0f);
            f3 history = mk3(r.col[0], r.col[1], r.col[2]);
            if (success)
            {
                float cv[3], ext[3], cen[3], mx = 0.0f;
                const float hv[3] = { history.x, history.y, history.z };
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    const float mean = s1[c] * (1.0f / 289.0f);
                    const float sd   = fm::sqrt1(fm::fmax_(s2[c] * (1.0f / 289.0f) - mean * mean, 0.0f));
                    // clip_aabb (:111-129) with aabb = mean -/+ sd: centre = mean, extent = sd + 0.001
                    cen[c] = mean; ext[c] = sd + 0.001f;
                    cv[c]  = hv[c] - mean;
                    mx     = fm::fmax_(mx, __builtin_fabsf(cv[c] * fm::rcp(ext[c])));
                }
                if (mx > 1.0f)
                {
                    const float im = fm::rcp(mx);
                    history = mk3(cen[0] + cv[0] * im, cen[1] + cv[1] * im, cen[2] + cv[2] * im);
                }
            }
            const float max_acc = a.moving ? 8.0f : hl;
            const float ia = fm::div_by_inrange(1.0f, div_prepare(max_acc));   // correctly rounded (1 <= max_acc <= 32): the moments' blend factor, see Reproj::resolve
            const float al = success ? fm::fmax_(a.alpha, ia) : 1.0f;
            const float am = success ? fm::fmax_(a.moments_alpha, ia) : 1.0f;
            const float lum = luminance(color);
            m0 = fm::mix_rn(r.mom[0], lum, am);
            m1 = fm::mix_rn(r.mom[1], lum * lum, am);
            r3 = fm::fmax_(0.0f, fm::var_rn(m1, m0));
            r0 = fm::mix_rn(history.x, color.x, al); r1 = fm::mix_rn(history.y, color.y, al); r2 = fm::mix_rn(history.z, color.z, al);
        }
        *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.out_moments) + o * 8u) = make_uint2(fm::pack2(m0, m1), fm::pack2(hl, 0.0f));
        *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.out) + o * 8u)         = make_uint2(fm::pack2(r0, r1), fm::pack2(r2, r3));
        // geometry record {oct normal, mesh id | linear z}: copies of the G-buffer's words, for this frame's a-trous taps and the next
        // frame's reprojection
        if (a.geo_out) *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.geo_out) + o * 8u) = make_uint2(cg2.x, cg3.y);
        if (d != 1.0f && roughness >= 0.05f) flag = (a.approximate_with_ddgi == 1) ? (roughness <= 0.75f) : true;
    }
    return live ? rp.near13 : 0u;
    };
    const uint32_t doubt = pixel(false);
    if (__any(doubt != 0u)) pixel(true);   // rare: the cold copy
    // tile classification per 8x8 tile (4 tiles per workgroup): :262-272
    if (flag) atomicOr(&s_flag[lx >> 3], 1);
    __syncthreads();
    if (threadIdx.x < 4)
    {
        const int tx = (bx0 >> 3) + threadIdx.x, ty = by0 >> 3;
        if (tx < a.tiles_x) a.tile_class[(size_t)ty * a.tiles_x + tx] = s_flag[threadIdx.x] ? 1 : 0;
    }
}

// reflections_denoise_atrous.comp + copy_tiles (tile class), tolerance mode
template <int STEP, bool N32>
__global__ __launch_bounds__(256) void kf_refl_atrous(ReflAtrousArgs a)
{
    const uint2 BLK = block_xy<0>();
    const int x = BLK.x * 32 + (threadIdx.x & 31), y = a.y0 + BLK.y * 8 + (threadIdx.x >> 5);
    if (x >= a.w || y >= a.y1) return;
    const uint32_t o = (uint32_t)(y * a.w + x);
    const uint2    c = fm::ld<uint2>(a.in.p, o * 8u);
    uint2          result = c;
    if (a.tile_class[(size_t)(y >> 3) * a.tiles_x + (x >> 3)])
    {
        const int  step = STEP > 0 ? STEP : a.step, R = STEP > 0 ? 1 : a.radius;
        const int  fx0 = (int)BLK.x * 32, fy0 = a.y0 + (int)BLK.y * 8, reach = step * R > 1 ? step * R : 1;
        const bool interior = fx0 - reach >= 0 && fx0 + 31 + reach < a.w && fy0 - reach >= a.in.y0 && fy0 + 7 + reach < a.in.y1;
        const f3    cc = refl_colour(c);
        const float center_luma = refl_luma(cc);
        float var = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++)
        {
            const int   xx = k % 3 - 1, yy = k / 3 - 1;
            const float kw = prefilter_weight(xx, yy);
            const uint32_t v = interior ? fm::ld<uint32_t>(a.in.p, (uint32_t)((y + yy) * a.w + (x + xx)) * 8u + 4u) : a.in.raw(x + xx, y + yy).y;
            var += fm::hi(v) * kw;
        }
        const uint32_t g2x = fm::ld<uint32_t>(a.gb2.p, o * 8u);
        const uint2    g3  = fm::ld<uint2>(a.gb3.p, o * 8u);
        const float    d = fm::ld<float>(a.depth.p, o * 4u), roughness = fm::lo(g3.x);
        if (d == 1.0f) result = make_uint2(0u, 0u);
        else if (!(roughness < 0.05f || (a.approximate_with_ddgi == 1 && roughness > 0.75f)))
        {
            const f3    cn = fm::oct_unit(g2x);
            const float center_depth = fm::hi(g3.y);
            EdgeK ek = edge_setup(a.sigma_depth, a.phi_normal, N32);
            ek.inv_phi_l = edge_luma(a.phi_color, var);
            float sum_w = 1.0f, s0 = cc.x, s1 = cc.y, s2 = cc.z, s3 = fm::hi(c.y);
            auto tap = [&](uint2 q, uint32_t q2x, uint32_t q3y, float kk, bool ok) {
                const f3    sc = refl_colour(q);
                const float sl = refl_luma(sc);
                float wc = fm::mul_rn(edge_weight_fast(ek, center_depth, fm::hi(q3y), cn, fm::oct_unit(q2x), center_luma, sl), kk);
                if (!ok) wc = 0.0f;
                sum_w += wc;
                s0 += wc * sc.x; s1 += wc * sc.y; s2 += wc * sc.z;
                s3 += (wc * wc) * fm::hi(q.y);
            };
            if (STEP > 0)
            {
                uint2    t_in[8];
                uint32_t t_g2[8], t_g3[8];
                bool     t_ok[8];
                if (interior)
                {
#pragma unroll
                    for (int t = 0; t < 8; t++)
                    {
                        const int      xx = tap_xy(t).xx, yy = tap_xy(t).yy;
                        const uint32_t so = (uint32_t)((y + yy * STEP) * a.w + (x + xx * STEP));
                        t_ok[t] = true;
                        t_in[t] = fm::ld<uint2>(a.in.p, so * 8u);
                        if (a.geo) { const uint2 q = fm::ld<uint2>(a.geo, so * 8u); t_g2[t] = q.x; t_g3[t] = q.y; }   // uniform branch
                        else { t_g2[t] = fm::ld<uint32_t>(a.gb2.p, so * 8u); t_g3[t] = fm::ld<uint32_t>(a.gb3.p, so * 8u + 4u); }
                    }
                }
                else
                {
#pragma unroll
                    for (int t = 0; t < 8; t++)
                    {
                        const int xx = tap_xy(t).xx, yy = tap_xy(t).yy;
                        const int px = x + xx * STEP, py = y + yy * STEP;
                        t_ok[t] = px >= 0 && py >= 0 && px < a.w && py < a.h;
                        t_in[t] = a.in.raw(px, py); t_g2[t] = a.gb2.raw(px, py).x; t_g3[t] = a.gb3.raw(px, py).y;
                    }
                }
#pragma unroll
                for (int t = 0; t < 8; t++)
                {
                    const int xx = tap_xy(t).xx, yy = tap_xy(t).yy;
                    tap(t_in[t], t_g2[t], t_g3[t], tap_weight(xx, yy), t_ok[t]);
                }
            }
            else
            {
                for (int yy = -R; yy <= R; yy++)
                    for (int xx = -R; xx <= R; xx++)
                    {
                        const int px = x + xx * step, py = y + yy * step;
                        if (px < 0 || py < 0 || px >= a.w || py >= a.h || (xx == 0 && yy == 0)) continue;
                        tap(a.in.raw(px, py), a.gb2.raw(px, py).x, a.gb3.raw(px, py).y, tap_weight(xx, yy), true);
                    }
            }
            const float iw = fm::rcp(sum_w);
            result = make_uint2(fm::pack2(s0 * iw, s1 * iw), fm::pack2(s2 * iw, s3 * (iw * iw)));
        }
    }
    *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.out) + o * 8u) = result;
    if (a.out2) *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.out2) + o * 8u) = result;
}


// Reflections a-trous iterations 0 and 1 in ONE launch (the scheme of kf_shadows_atrous01: A = tile + 4 staged once, iteration 0
// on B = tile + 3 rounded to RGBA16F as stored, iteration 1 on the tile).  Texel rules of kf_refl_atrous, texel by texel: outside
// the image -> weight 0 (staged with a zero normal); inside the image but outside the band's resident rows -> zeros that DO enter
// the sums (halo rows only), in both images; sky -> 0; copy tiles and mirror / DDGI-rough texels pass through.  Bit-identical to the
// two launches (tests/test_gpu_fused.py).
#ifndef FT_RATROUS01_ROWS
#define FT_RATROUS01_ROWS 1    // block_map.h block_xy<R>: tile rows per XCD run for the fused reflections a-trous 0 + 1 (0: identity, then HR_COLS8 bit 9 applies)
#endif
template <int TH, bool N32>
__global__ __launch_bounds__(256) void kf_refl_atrous01(ReflAtrousArgs a, uint2* out_first2)
{
    const uint2 BLK = block_xy<FT_RATROUS01_ROWS>();
    if ((int)BLK.x * 32 >= a.w) return;   // a padding column of the launch (block_map.h grid_cols)
    constexpr int AW = 38, AH = TH + 6, BW = 36, BH = TH + 4;   // A = tile + 3 all round, B = tile + 2 (round-3 advisor: one ring too many each)
    __shared__ uint2  s_in[AH * AW];
    __shared__ float4 s_nz[AH * AW];    // unit normal (0 outside the image), linear z
    __shared__ float  s_r[AH * AW];     // roughness; -1: sky texel
    __shared__ uint2  s_mid[BH * BW];
    const int bx0 = (int)BLK.x * 32, by0 = a.y0 + (int)BLK.y * TH;
    for (int i = threadIdx.x; i < AH * AW; i += 256)
    {
        const int  cy = i / AW, cx = i - cy * AW;
        const int  gx = bx0 - 3 + cx, gy = by0 - 3 + cy;
        const bool img = gx >= 0 && gx < a.w && gy >= 0 && gy < a.h;
        const bool res = img && gy >= a.in.y0 && gy < a.in.y1;
        const uint32_t so = res ? (uint32_t)(gy * a.w + gx) : (uint32_t)(a.in.y0 * a.w);
        uint2    c  = fm::ld<uint2>(a.in.p, so * 8u);
        uint32_t g2 = fm::ld<uint32_t>(a.gb2.p, so * 8u);
        uint2    g3 = fm::ld<uint2>(a.gb3.p, so * 8u);
        float    d  = fm::ld<float>(a.depth.p, so * 4u);
        if (!res) { c = make_uint2(0u, 0u); g2 = 0u; g3 = make_uint2(0u, 0u); d = 0.0f; }
        const f3 n = fm::oct_unit(g2);
        s_in[i] = c;
        s_nz[i] = img ? make_float4(n.x, n.y, n.z, fm::hi(g3.y)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_r[i]  = d == 1.0f ? -1.0f : fm::lo(g3.x);
    }
    __syncthreads();
    EdgeK ek = edge_setup(a.sigma_depth, a.phi_normal, N32);
    auto filter = [&](const uint2* img, int IW, int vi, int ci, int D) -> uint2 {
        const uint2 c = img[vi];
        const float roughness = s_r[ci];
        if (roughness == -1.0f) return make_uint2(0u, 0u);
        if (roughness < 0.05f || (a.approximate_with_ddgi == 1 && roughness > 0.75f)) return c;
        float var = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++)
        {
            const int   xx = k % 3 - 1, yy = k / 3 - 1;
            const float kw = prefilter_weight(xx, yy);
            var += fm::hi(img[vi + yy * IW + xx].y) * kw;
        }
        const float4 cnz = s_nz[ci];
        const f3     cn  = mk3(cnz.x, cnz.y, cnz.z);
        const f3     cc  = refl_colour(c);
        const float  center_luma = refl_luma(cc);
        ek.inv_phi_l = edge_luma(a.phi_color, var);
        float sum_w = 1.0f, s0 = cc.x, s1 = cc.y, s2 = cc.z, s3 = fm::hi(c.y);
#pragma unroll
        for (int t = 0; t < 8; t++)
        {
            const int    xx = tap_xy(t).xx, yy = tap_xy(t).yy;
            const float  kk = tap_weight(xx, yy);
            const uint2  q  = img[vi + yy * D * IW + xx * D];
            const float4 tn = s_nz[ci + yy * D * AW + xx * D];
            const f3     sc = refl_colour(q);
            const float  sl = refl_luma(sc);
            const float  wc = fm::mul_rn(edge_weight_fast(ek, cnz.w, tn.w, cn, mk3(tn.x, tn.y, tn.z), center_luma, sl), kk);
            sum_w += wc;
            s0 += wc * sc.x; s1 += wc * sc.y; s2 += wc * sc.z;
            s3 += (wc * wc) * fm::hi(q.y);
        }
        const float iw = fm::rcp(sum_w);
        return make_uint2(fm::pack2(s0 * iw, s1 * iw), fm::pack2(s2 * iw, s3 * (iw * iw)));
    };
    for (int j = threadIdx.x; j < BH * BW; j += 256)
    {
        const int  cy = j / BW, cx = j - cy * BW;
        const int  gx = bx0 - 2 + cx, gy = by0 - 2 + cy;
        const bool res = gx >= 0 && gx < a.w && gy >= (a.y0 > 0 ? a.y0 : 0) && gy < (a.y1 < a.h ? a.y1 : a.h);
        const int  ci = (cy + 1) * AW + cx + 1;
        uint2      r = make_uint2(0u, 0u);
        if (res) r = a.tile_class[(size_t)(gy >> 3) * a.tiles_x + (gx >> 3)] ? filter(s_in, AW, ci, ci, 1) : s_in[ci];
        s_mid[j] = r;
        if (out_first2 && res && cx >= 2 && cx < 34 && cy >= 2 && cy < 2 + TH) out_first2[(uint32_t)(gy * a.w + gx)] = r;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < TH * 32; j += 256)
    {
        const int lx = j & 31, ly = j >> 5, x = bx0 + lx, y = by0 + ly;
        if (x >= a.w || y >= a.y1) continue;
        const uint32_t o = (uint32_t)(y * a.w + x);
        const int vi = (ly + 2) * BW + lx + 2;
        const uint2 r = a.tile_class[(size_t)(y >> 3) * a.tiles_x + (x >> 3)] ? filter(s_mid, BW, vi, (ly + 3) * AW + lx + 3, 2) : s_mid[vi];
        a.out[o] = r;
        if (a.out2) a.out2[o] = r;
    }
}

} // namespace

namespace hr {

void launch_refl_temporal_fast(const ReflTemporalArgs& a_, hipStream_t st)
{
    ReflTemporalArgs a = a_;
    const dim3 grid = grid_with_sort(a.sort, grid_cols(cdiv(a.w, FR_TW), 6), cdiv(a.y1 - a.y0, FR_TH));
    if (a.geo_hist) hipLaunchKernelGGL(kf_refl_temporal<1>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(kf_refl_temporal<0>, grid, dim3(256), 0, st, a);
}

void launch_refl_atrous_fast(const ReflAtrousArgs& a, hipStream_t st)
{
    const dim3 grid(grid_cols(cdiv(a.w, 32), 1), cdiv(a.y1 - a.y0, 8));
    const bool n32 = a.phi_normal == 32.0f;
#define HR_LAUNCH_RATROUS(S) \
    do { if (n32) hipLaunchKernelGGL((kf_refl_atrous<S, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((kf_refl_atrous<S, false>), grid, dim3(256), 0, st, a); } while (0)
    if (a.radius == 1 && a.step == 1) HR_LAUNCH_RATROUS(1);
    else if (a.radius == 1 && a.step == 2) HR_LAUNCH_RATROUS(2);
    else if (a.radius == 1 && a.step == 4) HR_LAUNCH_RATROUS(4);
    else if (a.radius == 1 && a.step == 8) HR_LAUNCH_RATROUS(8);
    else HR_LAUNCH_RATROUS(0);
#undef HR_LAUNCH_RATROUS
}

#ifndef FT_RATROUS01_TH
#define FT_RATROUS01_TH 16
#endif
bool launch_refl_atrous01_fast(const ReflAtrousArgs& a, uint2* out_first2, hipStream_t st)
{
    if (a.radius != 1 || a.step != 1) return false;
    const dim3 grid(grid_cols(cdiv(a.w, 32), 9), cdiv(a.y1 - a.y0, FT_RATROUS01_TH));
    if (a.phi_normal == 32.0f) hipLaunchKernelGGL((kf_refl_atrous01<FT_RATROUS01_TH, true>), grid, dim3(256), 0, st, a, out_first2);
    else hipLaunchKernelGGL((kf_refl_atrous01<FT_RATROUS01_TH, false>), grid, dim3(256), 0, st, a, out_first2);
    return true;
}

} // namespace hr
