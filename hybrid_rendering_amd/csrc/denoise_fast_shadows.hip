// Tolerance-mode shadows denoiser: the temporal kernel and the a-trous chain (denoise_fast_common.h has what the passes share).
#include "denoise_fast_common.h"
#include "mask_window.h"
#include "tile_order.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// shadows_denoise_reprojection.comp:196-293 (+ reset_args / tile classification), tolerance mode
#ifndef FT_SHADOWS_EU
#define FT_SHADOWS_EU 6   // minimum waves per SIMD the register allocator must leave room for (round 5: 6 — with the cold copy of the pixel program 5 lets the allocator take 88 VGPRs; 6 = 80 VGPRs, three spill stores on the hot path).  Round 4, without the cold copy: 5 and 6 give the same 77 VGPRs (= 6 waves per SIMD), no
                          // spill: 48-50 us at 1080p, 208 at 4K; 7 (72 VGPRs + 24 B of scratch) 58.7 / 252.8; 8 (64 VGPRs, more scratch) 81.4 / 362 — spills
                          // cost far more than waves buy
#endif
// PATHS: TemporalPaths bits (pass_args.h) — forms of the first run's history loads; the cold copy keeps the form it had (its code and its
// registers stay what they were), and the outputs are the same bits
template <int GEO, int PATHS>
__global__ __launch_bounds__(64 * FT_WAVES, FT_SHADOWS_EU) void kf_shadows_temporal(TemporalArgs a)
{
    if (geo_apron_rides<64 * FT_WAVES>(a.apron)) return;   // row bands: the records of the history apron, as extra grid rows behind the sort's
    if (tile_order_rides<64 * FT_WAVES>(a.sort)) return;   // the trace kernel's next launch order, as extra grid rows (tile_order.h)
    const uint2 BLK = block_xy<0>();
    __shared__ uint32_t s_mask[FT_WAVES][1][18];
    __shared__ MaskRows s_rows[FT_WAVES];
    const int  lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // grid = (tile columns / FT_WAVES, tile rows): no integer division per wave
    const int  txr = BLK.x * FT_WAVES + wave;
    const bool tile_ok = txr < a.tiles_x;
    const int  tx = tile_ok ? txr : 0, ty = (int)BLK.y + a.tile_y0;
    const int  lx = lane & 7, ly = lane >> 3;
    const int  x = tx * 8 + lx, y = ty * 8 + ly;
    // order of the memory round trips: centre texels -> (mask words, LDS) -> history taps -> (popcounts) -> resolve
    const bool in_image = tile_ok && x < a.w && y < a.h && y >= a.y0 && y < a.y1;
    const bool edge     = tile_ok && (x >= a.w || y >= a.h);   // thread without a pixel: votes as the unguarded shader thread does
    const uint32_t pix  = in_image ? (uint32_t)(y * a.w + x) : (uint32_t)(a.y0 * a.w);
    const float d_raw   = fm::ld<float>(a.depth.p, pix * 4u);
    const uint2 cg2_raw = fm::ld<uint2>(a.gb2.p, pix * 8u), cg3_raw = fm::ld<uint2>(a.gb3.p, pix * 8u);
    build_mask_rows<false>(s_rows[wave], s_mask[wave], a.mask, 1, a.mw, a.mh, tx, ty, a.y0, a.y1, lane, tile_ok);
    if (!tile_ok) return;
    // The pixel's program, from its centre texels on.  It runs once; a wave in which some history tap sat on a knife edge of the validity
    // test (Reproj::tap_valid notes it: a handful of pixels per frame) runs it a SECOND time — a second, cold copy of the code, entered with
    // nothing of the first run live — in which the noted pixels take the parity kernels' verdicts on their taps (Reproj::exact_bits), and
    // stores again.  Returns near13 (0: no tap of this pixel was in doubt); flag = the pixel's vote in the tile classification.
    bool flag = false;
    auto pixel = [&](const float d_in, const uint2 cg2_in, const uint2 cg3_in, auto redo_c) -> uint32_t {
        constexpr bool redo = decltype(redo_c)::value;
        const float d   = edge ? 0.0f : d_in;
        const uint2 cg2 = edge ? make_uint2(0u, 0u) : cg2_in, cg3 = edge ? make_uint2(0u, 0u) : cg3_in;
        const f3    cn  = fm::oct_unit(cg2.x);
        const bool  live = (in_image || edge) && d != 1.0f;
        Reproj<4, true, false, GEO, redo ? 0 : PATHS> rp;
        rp.M = a.vpi; rp.pgb2 = a.pgb2.p; rp.pgb3 = a.pgb3.p; rp.pdepth = a.pdepth.p; rp.hist = a.hist.p; rp.hist_moments = a.hist_moments.p; rp.hist_len = nullptr;
        rp.geo = a.geo_hist;
        rp.g = HistGeom { a.w, a.h, a.pgb2.y0, a.pgb2.y1 };
        const bool reproj = live && !a.debug_skip_reproject;
        uint32_t ovr = 0u, known = 0u;
        if (redo && reproj)
        {
            // Which taps were in doubt is found again the way the first run found it (the fast test is deterministic); THOSE taps get the parity
            // kernels' verdicts (typically one tap: ~250 VALU instead of 3250 for all 13).  If that changes the verdict of a bilinear tap, the
            // 3x3 fallback may run where it did not before (or the other way round) and its taps were never tested for doubt: then all nine
            // get exact verdicts as well.  Straight-line code on purpose: as a loop ("until nothing new is noted") the allocator spilled on
            // the HOT path (+13 %, docs/EXPERIMENTS.md R5.1).
            rp.issue(x, y, d, cg2.y, fm::lo(cg3.y), 0.0f, cn, mk3(0, 0, 0), nullptr, 0.0f);
            ReprojOut r0;
            rp.template resolve<true>(r0);
            if (rp.near13)
            {
                known = rp.near13;
                ovr   = rp.exact_bits(known, x, y, d, cg2.x, cg2.y);
                if ((((ovr ^ rp.valid13) & known) & 0xfu) != 0u)   // a bilinear verdict flipped
                {
                    const uint32_t rest = 0x1ff0u & ~known;
                    ovr |= rp.exact_bits(rest, x, y, d, cg2.x, cg2.y);
                    known |= rest;
                }
            }
        }
        if (reproj) rp.issue(x, y, d, cg2.y, fm::lo(cg3.y), 0.0f, cn, mk3(0, 0, 0), nullptr, 0.0f);
        if (!redo && a.apron_flag && __ballot(reproj && in_image && y >= a.band_y0 && y < a.band_y1 && rp.apron_miss) && lane == 0) atomicOr(a.apron_flag, 1u);
        int sum, own;
        mask_window<false>(s_rows[wave], lx, ly, sum, own);   // 17 bfe + bcnt pairs while the 21 history loads are in flight
        const float mean = fm::div_by_inrange((float)sum, div_prepare(289.0f));

        float out_v = 0.0f, out_var = 0.0f, m0 = 0.0f, m1 = 0.0f, hlen = 0.0f;
        flag = false;
        rp.near13 = 0u;
        if (live)
        {
            const float visibility = (float)own;
            ReprojOut   r;
            bool        success = false;
            if (reproj) success = rp.template resolve<true>(r, ovr, known);
            else { r.col[0] = 0.0f; r.mom[0] = r.mom[1] = 0.0f; r.length = 0.0f; }
            hlen = fm::fmin_(32.0f, success ? r.length + 1.0f : 1.0f);
            float hv = r.col[0];
            if (success)
            {
                const float sd = fm::sqrt1(fm::fmax_(fm::var_rn(mean, mean), 0.0f));
                hv = fm::fmin_(fm::fmax_(hv, mean - 0.5f * sd), mean + 0.5f * sd);
            }
            const float ih = fm::rcp_nr(hlen);
            const float al = success ? fm::fmax_(a.alpha, ih) : 1.0f;
            const float am = success ? fm::fmax_(a.moments_alpha, ih) : 1.0f;
            m0      = fm::mix_rn(r.mom[0], visibility, am);
            m1      = fm::mix_rn(r.mom[1], visibility * visibility, am);
            out_var = fm::fmax_(0.0f, fm::var_rn(m1, m0));
            out_v   = fm::mix_rn(hv, visibility, al);
            flag    = out_v > 0.0f;
        }
        if (in_image)
        {
            *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.out_moments) + pix * 8u) = make_uint2(fm::pack2(m0, m1), fm::pack2(hlen, 0.0f));
            // for the a-trous iterations: the centre's octahedral normal and linear depth, 8 bytes (copies of the G-buffer's fp16 values —
            // the exact mode keeps 16 bytes of decoded fp32; decoding per tap is cheaper than the extra 8 B x 5 passes of HBM traffic)
            *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.nd) + pix * 8u)         = make_uint2(cg2.x, cg3.y);
            *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out) + pix * 4u)     = fm::pack2(out_v, out_var);
        }
        return reproj ? rp.near13 : 0u;
    };
    const uint32_t doubt = pixel(d_raw, cg2_raw, cg3_raw, BoolC<false>());
    if (__any(doubt != 0u))   // rare: the cold copy (re-reads the centre texels: nothing of the first run is kept)
        pixel(fm::ld<float>(a.depth.p, pix * 4u), fm::ld<uint2>(a.gb2.p, pix * 8u), fm::ld<uint2>(a.gb3.p, pix * 8u), BoolC<true>());
    const unsigned long long any = __ballot(flag);
    if (lane == 0) a.tile_class[(size_t)ty * a.tiles_x + tx] = any ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// shadows_denoise_atrous.comp:94-174 + copy_shadow_tiles (tile class), tolerance mode.  STEP > 0: compile-time tap distance and
// radius 1 (the reference default, fully unrolled: atrous_gather_pixel); STEP == 0: run-time step and radius.  The filter itself is
// atrous_filters.h.
//
// One pixel of a live tile for kf_shadows_atrous<STEP > 0>: every load first, in one batch, then the arithmetic.  INTERIOR: the
// workgroup's whole footprint is resident, no bounds test; else a texel that is not resident is fetched at the centre's address
// and counts as 0 (variance) / gets weight 0 (tap).  Two whole copies of the pixel on purpose: with only the loads in the two
// branches the compiler merges the geometry loads behind the join and waits for the value loads before it issues them.
template <int STEP, bool N32, bool INTERIOR>
HR_DEV void atrous_gather_pixel(const AtrousArgs& a, int x, int y, uint32_t o)
{
    uint32_t v_in[9], t_in[8];
    uint2    t_nd[8];
    bool     t_ok[8];
    const uint32_t c   = fm::ld<uint32_t>(a.in.p, o * 4u);
    const uint2    cnd = fm::ld<uint2>(a.nd, o * 8u);   // oct normal (fp16 x 2), mesh id | linear z (fp16 x 2)
#pragma unroll
    for (int k = 0; k < 9; k++)
    {
        const int xx = k % 3 - 1, yy = k / 3 - 1, px = x + xx, py = y + yy;
        if (k == 4) { v_in[k] = c; continue; }
        if (INTERIOR) v_in[k] = fm::ld<uint32_t>(a.in.p, (uint32_t)(py * a.w + px) * 4u);
        else
        {
            const bool     res = px >= 0 && px < a.w && py >= a.y0 && py < a.y1;   // a texel that is not resident is 0 (ImgRG16F::raw)
            const uint32_t vv  = fm::ld<uint32_t>(a.in.p, (res ? (uint32_t)(py * a.w + px) : o) * 4u);
            v_in[k] = res ? vv : 0u;
        }
    }
#pragma unroll
    for (int t = 0; t < 8; t++)
    {
        const int px = x + tap_xy(t).xx * STEP, py = y + tap_xy(t).yy * STEP;
        // a tap outside the image is skipped; one outside the resident rows of a band reads zeros, whose weight is 0 (halo
        // rows only): both get weight 0 below
        const bool     res = INTERIOR || (px >= 0 && py >= 0 && px < a.w && py < a.h && py >= a.y0 && py < a.y1);
        const uint32_t so  = res ? (uint32_t)(py * a.w + px) : o;
        t_ok[t] = res;
        t_in[t] = fm::ld<uint32_t>(a.in.p, so * 4u);
        t_nd[t] = fm::ld<uint2>(a.nd, so * 8u);
    }
    __builtin_amdgcn_sched_barrier(0);   // nothing of the arithmetic (and none of its waits) in front of a load
    // the texel source: those register arrays, decoded at use
    struct Loaded
    {
        const uint32_t (&v_in)[9], (&t_in)[8];
        const uint2    (&t_nd)[8], cnd;
        const bool     (&t_ok)[8];
        static HR_DEV constexpr int k(int xx, int yy) { return (yy + 1) * 3 + (xx + 1); }
        static HR_DEV constexpr int t(int xx, int yy) { return k(xx, yy) < 4 ? k(xx, yy) : k(xx, yy) - 1; }
        HR_DEV uint32_t unit(int xx, int yy) const { return v_in[k(xx, yy)]; }
        HR_DEV uint32_t tap(int xx, int yy) const { return t_in[t(xx, yy)]; }
        HR_DEV NZ       nz(int xx, int yy) const { return (xx == 0 && yy == 0) ? nz_of(cnd.x, cnd.y) : nz_of(t_nd[t(xx, yy)].x, t_nd[t(xx, yy)].y); }
        HR_DEV bool     ok(int xx, int yy) const { return t_ok[t(xx, yy)]; }
    };
    // a sky centre passes through by select: its taps were fetched for nothing
    const uint32_t result = shadows_filter<false>(Loaded { v_in, t_in, t_nd, cnd, t_ok }, [&] { return edge_setup(a.sigma_depth, a.phi_normal, N32); }, a.phi_visibility, a.power);
    *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out) + o * 4u) = result;
    if (a.out2) *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out2) + o * 4u) = result;
}

// Per-wave record of the instrumented kernels kf_shadows_atrous_timeline / kf_shadows_atrous01_timeline (developer switch
// HR_DEBUG_ATROUS_TIMELINE, tools/atrous_balance.py), the way k_shadows_trace fills TraceArgs::timeline: register reads only.  They run the
// bodies of kf_shadows_atrous<4 | 8> / kf_shadows_atrous01, which return whether the workgroup was live (had a tile that is no shadow tile);
// the default kernels drop that value and hold none of this.
struct AtrousTimeline
{
    unsigned long long t_begin;
    HR_DEV AtrousTimeline() : t_begin(wall_clock64()) {}
    HR_DEV void exit(unsigned long long* timeline, int live) const
    {
        if (!timeline || (threadIdx.x & 63u)) return;
        const unsigned long long t_end = wall_clock64();
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        const size_t slot = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4u + (threadIdx.x >> 6);   // four waves per workgroup
        timeline[slot * 4 + 0] = t_begin;
        timeline[slot * 4 + 1] = t_end;
        timeline[slot * 4 + 2] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
        timeline[slot * 4 + 3] = (unsigned long long)live;
    }
};

template <int STEP, bool N32>
HR_DEV int shadows_atrous_body(const AtrousArgs& a)
{
    const uint2 BLK = block_xy<0>();
    if constexpr (STEP > 0)
    {
        // Radius 1, compile-time tap distance: ONE vector round trip per live wave (it was three: tile class -> centre -> taps).  The
        // classes of the workgroup's four tiles (32 x 8 pixels = four tiles of one tile row; a.y0 is a multiple of 8) come through a
        // wave-uniform fetch — the two aligned dwords that hold the four bytes, shifted: the class image is readable 8 bytes past its
        // last tile — and every texel the pixel needs (centre, 3x3 variance, 8 taps: value + geometry record) is then requested at
        // once, at addresses that are resident whatever the centre turns out to be; a sky centre (linear z < 0: rare inside a live
        // tile) throws its taps away afterwards.
        const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
        const int fx0 = (int)BLK.x * 32, fy0 = a.y0 + (int)BLK.y * 8;
        if (fx0 >= a.w) return 0;   // a padding column of the launch (block_map.h grid_cols)
        const uint32_t  tb   = (uint32_t)(fy0 >> 3) * (uint32_t)a.tiles_x + (uint32_t)(fx0 >> 3);
        const uint32_t* tc   = reinterpret_cast<const uint32_t*>(a.tile_class) + (tb >> 2);
        const uint32_t  cls4 = (uint32_t)(((uint64_t)tc[0] | ((uint64_t)tc[1] << 32)) >> ((tb & 3u) * 8u));
        const int live = (cls4 & (a.tiles_x - (fx0 >> 3) >= 4 ? 0xffffffffu : (1u << ((a.tiles_x - (fx0 >> 3)) * 8)) - 1u)) ? 1 : 0;   // for the timeline only
        const int x = fx0 + lx, y = fy0 + ly;
        if (x >= a.w || y >= a.y1) return live;
        const uint32_t o = (uint32_t)(y * a.w + x);
        if (!((cls4 >> ((lx >> 3) * 8)) & 0xffu))
        {
            *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out) + o * 4u) = 0u; // shadows_denoise_copy_shadow_tiles.comp:35
            if (a.out2) *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out2) + o * 4u) = 0u;
            return live;
        }
        // a workgroup whose whole footprint lies inside the resident rows needs no bounds test at all (uniform branch)
        const bool interior = fx0 - STEP >= 0 && fx0 + 31 + STEP < a.w && fy0 - STEP >= (a.y0 > 0 ? a.y0 : 0) && fy0 + 7 + STEP < (a.y1 < a.h ? a.y1 : a.h);
        if (interior) atrous_gather_pixel<STEP, N32, true>(a, x, y, o);
        else atrous_gather_pixel<STEP, N32, false>(a, x, y, o);
        return live;
    }
    // STEP == 0: run-time tap distance and radius
    const int x = BLK.x * 32 + (threadIdx.x & 31);
    const int y = a.y0 + BLK.y * 8 + (threadIdx.x >> 5);
    if (x >= a.w || y >= a.y1) return 1;
    const uint32_t o = (uint32_t)(y * a.w + x);
    uint32_t* outp  = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out) + o * 4u);
    uint32_t* out2p = a.out2 ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out2) + o * 4u) : nullptr;
    if (!a.tile_class[(size_t)(y >> 3) * a.tiles_x + (x >> 3)])
    {
        *outp = 0u; // shadows_denoise_copy_shadow_tiles.comp:35
        if (out2p) *out2p = 0u;
        return 1;
    }
    const int step = a.step, R = a.radius;
    // a workgroup whose whole footprint lies inside the resident rows needs no bounds test at all (uniform branch)
    const int  fx0 = (int)BLK.x * 32, fy0 = a.y0 + (int)BLK.y * 8;
    const int  reach = step * R > 1 ? step * R : 1;
    const bool interior = fx0 - reach >= 0 && fx0 + 31 + reach < a.w && fy0 - reach >= (a.y0 > 0 ? a.y0 : 0) && fy0 + 7 + reach < (a.y1 < a.h ? a.y1 : a.h);
    const uint32_t c   = fm::ld<uint32_t>(a.in.p, o * 4u);
    const uint2    cnd = fm::ld<uint2>(a.nd, o * 8u);   // oct normal (fp16 x 2), mesh id | linear z (fp16 x 2)
    const float    cz  = fm::hi(cnd.y);
    // compute_variance_center (:65-88): 3x3 gaussian of the variance channel, unit taps
    const float var = interior ? prefilter_variance([=](int xx, int yy) { return fm::hi(fm::ld<uint32_t>(a.in.p, (uint32_t)((y + yy) * a.w + (x + xx)) * 4u)); })
                               : prefilter_variance([=](int xx, int yy) { return fm::hi(a.in.raw(x + xx, y + yy)); });
    uint32_t result = c;
    if (!(cz < 0.0f))
    {
        const NZ    cnz = nz_of(cnd.x, cnd.y);
        const float cv  = fm::lo(c);
        EdgeK ek = edge_setup(a.sigma_depth, a.phi_normal, N32);
        ek.inv_phi_l = edge_luma(a.phi_visibility, var);
        ShadowSums sum { 1.0f, cv, fm::hi(c) };
        for (int yy = -R; yy <= R; yy++)
            for (int xx = -R; xx <= R; xx++)
            {
                const int px = x + xx * step, py = y + yy * step;
                if (px < 0 || py < 0 || px >= a.w || py >= a.h || (xx == 0 && yy == 0)) continue;
                const float kk = tap_weight(xx, yy);
                if (py < a.y0 || py >= a.y1) continue;   // outside the resident rows of a band: zeros, weight 0
                const uint32_t so = (uint32_t)(py * a.w + px);
                const uint32_t s  = fm::ld<uint32_t>(a.in.p, so * 4u);
                const uint2    nd = fm::ld<uint2>(a.nd, so * 8u);
                sum.add(ek, cnz, cv, nz_of(nd.x, nd.y), s, kk, true);
            }
        result = sum.finish(a.power);
    }
    *outp = result;
    if (out2p) *out2p = result;
    return 1;
}

template <int STEP, bool N32>
__global__ __launch_bounds__(256) void kf_shadows_atrous(AtrousArgs a)
{
    (void)shadows_atrous_body<STEP, N32>(a);
}

template <int STEP>
__global__ __launch_bounds__(256) void kf_shadows_atrous_timeline(AtrousArgs a, unsigned long long* timeline)
{
    const AtrousTimeline tl;
    const int live = shadows_atrous_body<STEP, true>(a);
    tl.exit(timeline, live);
}


// The same filter with its taps staged through LDS (radius 1, tap distance STEP = 1 / 2 / 4 / 8: the reference's four iterations).
// The 32x8 tile and its STEP-wide apron are fetched ONCE per workgroup — (32+2S)x(8+2S) texels instead of 27 loads per pixel, which
// had the kernel bound by the L1 data path, not by HBM or the VALU (SQ counters: 38 % VALU busy, counter traffic 27-40 MB) — and
// each texel's octahedral normal is decoded once instead of once per tap that reads it.  A texel that is not resident (outside the
// image or the band's rows) is staged as (value 0, normal 0): its edge weight is exactly 0 (pow(dot(n, 0), phi) = 0).
// How the staged kernels (kf_shadows_atrous_lds, kf_shadows_atrous01) read global memory: a workgroup's whole staged tile in one batch
// of loads (atrous_filters.h ShadowsStageBatch), and kf_shadows_atrous01's vote from wave-uniform dwords.  The loops and the vote they
// replaced — a round trip per value, per geometry record and per round, and one plus a barrier for the vote — and each part's time:
// docs/EXPERIMENTS.md, "Shadow a-trous 0+1: the staging in one round trip".
template <int STEP, bool N32>
__global__ __launch_bounds__(256) void kf_shadows_atrous_lds(AtrousArgs a)
{
    const uint2 BLK = block_xy<0>();
    constexpr int TW = 32 + 2 * STEP, TH = 8 + 2 * STEP;
    __shared__ uint32_t s_in[TH * TW];
    __shared__ float4   s_nz[TH * TW];   // unit normal, linear z
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int bx0 = (int)BLK.x * 32, by0 = a.y0 + (int)BLK.y * 8;
    if (bx0 >= a.w) return;   // a padding column of the launch (block_map.h grid_cols)
    const int x = bx0 + lx, y = by0 + ly;
    const bool inside = x < a.w && y < a.y1;
    const uint32_t cls = inside ? a.tile_class[(size_t)(y >> 3) * a.tiles_x + (x >> 3)] : 0u;
    if (__syncthreads_or((int)cls))   // a workgroup of shadow tiles only stages nothing (staging unconditionally: 14.4 -> 17.8 µs at step 1)
    {
        const int ry0 = a.y0 > 0 ? a.y0 : 0, ry1 = a.y1 < a.h ? a.y1 : a.h;
        ShadowsStageBatch<(TH * TW + 255) / 256, TW, TH * TW> batch;   // the tile in one round trip
        batch.load(a, bx0 - STEP, by0 - STEP, ry0, ry1);
        __builtin_amdgcn_sched_barrier(0);
        batch.store(s_in, s_nz);
        __syncthreads();
    }
    if (!inside) return;
    const uint32_t o = (uint32_t)(y * a.w + x);
    uint32_t* outp  = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out) + o * 4u);
    uint32_t* out2p = a.out2 ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.out2) + o * 4u) : nullptr;
    if (!cls)
    {
        *outp = 0u; // shadows_denoise_copy_shadow_tiles.comp:35
        if (out2p) *out2p = 0u;
        return;
    }
    const int      ci     = (ly + STEP) * TW + (lx + STEP);
    const uint32_t result = shadows_filter<true>(StagedTaps { s_in, s_nz, TW, ci, TW, ci, STEP }, [&] { return edge_setup(a.sigma_depth, a.phi_normal, N32); }, a.phi_visibility, a.power);
    *outp = result;
    if (out2p) *out2p = result;
}

// A-trous iterations 0 and 1 (tap distances 1 and 2, radius 1) in ONE launch: iteration 0's image never leaves LDS.
// Per 32 x TH output tile: region A = the tile + 3 texels all round is staged once (value/variance + decoded normal + linear z);
// iteration 0 runs on region B = the tile + 2 (iteration 1 reads B at distance 2 for its taps, at distance 1 around the centre only for its
// 3x3 variance prefilter; iteration 0 reads A at distance 1) and
// is rounded to RG16F exactly as the stored image would be; iteration 1 runs on the tile.  Saves one launch, one 4 B/px image write
// and the second pass's re-fetch of the 8 B/px normal/depth image at the cost of (B + tile) / (2 tile) filter evaluations.
// Texel rules are those of kf_shadows_atrous_lds: a texel outside the image / the band's resident rows is (0, normal 0) in BOTH
// images (weight exactly 0), a texel of a shadow tile is 0 after iteration 0 (copy_shadow_tiles.comp), so the result is
// bit-identical to the two launches (tests/test_gpu_fused.py).  a.out2 = feedback copy of iteration 1, a.out_first2 = of iteration 0.
// Global reads of a workgroup: the classes of its own 4 x (TH / 8) tiles as wave-uniform dwords (a workgroup of shadow tiles writes its
// zeros and leaves after that, with no vector load and no barrier), then region A in ONE batch — four texels per thread, value and
// geometry record, eight loads with nothing waiting between them (the parent: eight dependent round trips) — then one class byte per
// round of the two filter loops (five rounds; keeping the classes of the 6 x (TH / 8 + 2) reachable tiles in LDS instead was measured
// twice and is worth 0.2 µs: docs/EXPERIMENTS.md, "Shadow a-trous 0+1: the staging in one round trip").  tests/test_gpu_atrous01_staging.py.
template <int TH, bool N32>
HR_DEV int shadows_atrous01_body(const AtrousArgs& a, uint32_t* out_first2, float power1)
{
    const uint2 BLK = block_xy<0>();
    constexpr int AW = 38, AH = TH + 6, BW = 36, BH = TH + 4;   // A = tile + 3 all round, B = tile + 2 (round-3 advisor: one ring too many each)
    __shared__ uint32_t s_in[AH * AW];
    __shared__ float4   s_nz[AH * AW];   // unit normal, linear z
    __shared__ uint32_t s_mid[BH * BW];  // iteration 0, as the RG16F image would hold it
    const int bx0 = (int)BLK.x * 32, by0 = a.y0 + (int)BLK.y * TH;
    if (bx0 >= a.w) return 0;   // a padding column of the launch (block_map.h grid_cols)
    const int ry0 = a.y0 > 0 ? a.y0 : 0, ry1 = a.y1 < a.h ? a.y1 : a.h;
    // tile classes of this workgroup's own tiles: all shadow => every output is 0 and nothing is staged
    // wave-uniform, as in kf_shadows_atrous<STEP > 0>: per tile row the two aligned dwords that hold its four bytes, shifted.  No vector
    // round trip and no barrier in front of the decision.  A tile row is read only if its first pixel row lies above ry1 <= h, that is if
    // it exists, so the reads end at most 8 bytes past the last tile (hr_shadows_create allocates those) for the second tile row as for
    // the first; the columns past tiles_x are masked off.
    uint32_t any_cls = 0u;
    {
        const uint32_t cols = a.tiles_x - (bx0 >> 3) >= 4 ? 0xffffffffu : (1u << ((a.tiles_x - (bx0 >> 3)) * 8)) - 1u;
#pragma unroll
        for (int r = 0; r < TH / 8; r++)
        {
            const bool      row  = by0 + 8 * r < ry1;
            const uint32_t  tb   = (uint32_t)((by0 >> 3) + (row ? r : 0)) * (uint32_t)a.tiles_x + (uint32_t)(bx0 >> 3);
            const uint32_t* tc   = reinterpret_cast<const uint32_t*>(a.tile_class) + (tb >> 2);
            const uint32_t  cls4 = (uint32_t)(((uint64_t)tc[0] | ((uint64_t)tc[1] << 32)) >> ((tb & 3u) * 8u));
            any_cls |= row ? (cls4 & cols) : 0u;
        }
    }
    if (!any_cls)
    {
        for (int j = threadIdx.x; j < TH * 32; j += 256)
        {
            const int x = bx0 + (j & 31), y = by0 + (j >> 5);
            if (x >= a.w || y >= a.y1) continue;
            const uint32_t o = (uint32_t)(y * a.w + x);
            a.out[o] = 0u;
            if (a.out2) a.out2[o] = 0u;
            if (out_first2) out_first2[o] = 0u;
        }
        return 0;
    }
    // region A, requested at once: four texels per thread, value + geometry record
    ShadowsStageBatch<(AH * AW + 255) / 256, AW, AH * AW> batch;
    batch.load(a, bx0 - 3, by0 - 3, ry0, ry1);
    __builtin_amdgcn_sched_barrier(0);   // nothing of the decode (and none of its waits) in front of a load
    batch.store(s_in, s_nz);
    __syncthreads();
    const EdgeK ek = edge_setup(a.sigma_depth, a.phi_normal, N32);
    // one filter evaluation: centre index ci in the A grid, values from `img` (stride IW, centre index vi), taps at distance D
    auto filter = [&](const uint32_t* img, int IW, int vi, int ci, int D, float power) -> uint32_t {
        return shadows_filter<true>(StagedTaps { img, s_nz, IW, vi, AW, ci, D }, [&] { return ek; }, a.phi_visibility, power);
    };
    // iteration 0 on region B
    for (int j = threadIdx.x; j < BH * BW; j += 256)
    {
        const int  cy = j / BW, cx = j - cy * BW;
        const int  gx = bx0 - 2 + cx, gy = by0 - 2 + cy;
        const bool res = gx >= 0 && gx < a.w && gy >= ry0 && gy < ry1;
        uint32_t   r = 0u;
        if (res && a.tile_class[(size_t)(gy >> 3) * a.tiles_x + (gx >> 3)])
        {
            const int ci = (cy + 1) * AW + cx + 1;
            r = filter(s_in, AW, ci, ci, 1, 0.0f);
        }
        s_mid[j] = r;
        if (out_first2 && res && cx >= 2 && cx < 34 && cy >= 2 && cy < 2 + TH && gy < a.y1) out_first2[(uint32_t)(gy * a.w + gx)] = r;
    }
    __syncthreads();
    // iteration 1 on the tile
    for (int j = threadIdx.x; j < TH * 32; j += 256)
    {
        const int lx = j & 31, ly = j >> 5, x = bx0 + lx, y = by0 + ly;
        if (x >= a.w || y >= a.y1) continue;
        const uint32_t o = (uint32_t)(y * a.w + x);
        uint32_t r = 0u;
        if (a.tile_class[(size_t)(y >> 3) * a.tiles_x + (x >> 3)]) r = filter(s_mid, BW, (ly + 2) * BW + lx + 2, (ly + 3) * AW + lx + 3, 2, power1);
        a.out[o] = r;
        if (a.out2) a.out2[o] = r;
    }
    return 1;
}

template <int TH, bool N32>
__global__ __launch_bounds__(256) void kf_shadows_atrous01(AtrousArgs a, uint32_t* out_first2, float power1)
{
    (void)shadows_atrous01_body<TH, N32>(a, out_first2, power1);
}

template <int TH>
__global__ __launch_bounds__(256) void kf_shadows_atrous01_timeline(AtrousArgs a, uint32_t* out_first2, float power1, unsigned long long* timeline)
{
    const AtrousTimeline tl;
    const int live = shadows_atrous01_body<TH, true>(a, out_first2, power1);
    tl.exit(timeline, live);
}

} // namespace

namespace hr {

void launch_shadows_temporal_fast(const TemporalArgs& a_, int n_tiles, hipStream_t st)
{
    TemporalArgs a = a_;
    const dim3 grid = grid_with_apron(grid_with_sort(a.sort, grid_cols(cdiv(a.tiles_x, FT_WAVES), 4), a.tiles_y), a.apron, 64 * FT_WAVES);
    // the paired history loads (TemporalPaths) apply on the record path; a pair of texels needs two columns
    if (!a.geo_hist) hipLaunchKernelGGL((kf_shadows_temporal<0, 0>), grid, dim3(64 * FT_WAVES), 0, st, a);
    else if ((a.paths & TP_PAIRS) && a.w >= 2) hipLaunchKernelGGL((kf_shadows_temporal<1, TP_PAIRS>), grid, dim3(64 * FT_WAVES), 0, st, a);
    else hipLaunchKernelGGL((kf_shadows_temporal<1, 0>), grid, dim3(64 * FT_WAVES), 0, st, a);
}

void launch_shadows_atrous_fast(const AtrousArgs& a, hipStream_t st, unsigned long long* timeline)
{
    const dim3 grid(grid_cols(cdiv(a.w, 32), a.step >= 4 ? 0 : 7), cdiv(a.y1 - a.y0, 8));
    const bool n32 = a.phi_normal == 32.0f;
    if (timeline && n32 && a.radius == 1 && (a.step == 4 || a.step == 8))   // developer switch HR_DEBUG_ATROUS_TIMELINE: the instrumented kernel
    {
        if (a.step == 4) hipLaunchKernelGGL((kf_shadows_atrous_timeline<4>), grid, dim3(256), 0, st, a, timeline);
        else hipLaunchKernelGGL((kf_shadows_atrous_timeline<8>), grid, dim3(256), 0, st, a, timeline);
        return;
    }
#define HR_LAUNCH_ATROUS(K, S) \
    do { if (n32) hipLaunchKernelGGL((K<S, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((K<S, false>), grid, dim3(256), 0, st, a); } while (0)
    // tap distances 1 and 2 through LDS (apron 1-2 texels: 14.4 / 14.6 µs against 15.8 / 15.9 for per-pixel gathers at 1080p, event
    // times); at 4 and 8 the apron is as large as the tile and the gathers win (15.7 / 18.7 against 16.1 / 15.9)
    if (a.radius == 1 && a.step == 1) HR_LAUNCH_ATROUS(kf_shadows_atrous_lds, 1);
    else if (a.radius == 1 && a.step == 2) HR_LAUNCH_ATROUS(kf_shadows_atrous_lds, 2);
    else if (a.radius == 1 && a.step == 4) HR_LAUNCH_ATROUS(kf_shadows_atrous, 4);
    else if (a.radius == 1 && a.step == 8) HR_LAUNCH_ATROUS(kf_shadows_atrous, 8);
    else HR_LAUNCH_ATROUS(kf_shadows_atrous, 0);
#undef HR_LAUNCH_ATROUS
}

#ifndef FT_ATROUS01_TH
#define FT_ATROUS01_TH 16
#endif
// iterations 0 + 1 in one launch; `a` describes iteration 0 (a.in = temporal output, a.step == 1), a.out = the image iteration 1
// writes, a.out2 / out_first2 = the feedback copy of iteration 1 / 0, power1 = iteration 1's power.  false: not available
// lds_pad: bytes of unused dynamic LDS on top of the kernel's own, which bound how many of its workgroups a CU holds (pass_core.h
// atrous_resident_pad); timeline: nullptr, or the records of the instrumented kernel (developer switch HR_DEBUG_ATROUS_TIMELINE)
bool launch_shadows_atrous01_fast(const AtrousArgs& a, uint32_t* out_first2, float power1, hipStream_t st, int lds_pad, unsigned long long* timeline)
{
    if (a.radius != 1 || a.step != 1) return false;
    const dim3   grid(grid_cols(cdiv(a.w, 32), 7), cdiv(a.y1 - a.y0, FT_ATROUS01_TH));
    const size_t pad = lds_pad > 0 ? (size_t)lds_pad : 0;
    if (a.phi_normal != 32.0f) hipLaunchKernelGGL((kf_shadows_atrous01<FT_ATROUS01_TH, false>), grid, dim3(256), pad, st, a, out_first2, power1);
    else if (timeline) hipLaunchKernelGGL((kf_shadows_atrous01_timeline<FT_ATROUS01_TH>), grid, dim3(256), pad, st, a, out_first2, power1, timeline);
    else hipLaunchKernelGGL((kf_shadows_atrous01<FT_ATROUS01_TH, true>), grid, dim3(256), pad, st, a, out_first2, power1);
    return true;
}

// static LDS of kf_shadows_atrous01, for the pad (once, at create); < 0: unknown
int shadows_atrous01_static_lds()
{
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&kf_shadows_atrous01<FT_ATROUS01_TH, true>)) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (int)fa.sharedSizeBytes;
}
// workgroups of the largest grid either launcher makes for these arguments (the timeline buffer's size)
int shadows_atrous_max_workgroups(const AtrousArgs& a)
{
    return (cdiv(a.w, 32) + 8) * cdiv(a.y1 - a.y0, 8);
}

} // namespace hr
