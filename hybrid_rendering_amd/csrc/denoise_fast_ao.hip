// Tolerance-mode AO denoiser: the temporal kernel and the bilateral blurs (denoise_fast_common.h has what the passes share).
#include "denoise_fast_common.h"
#include "mask_window.h"
#include "tile_order.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// ao_denoise_reprojection.comp:191-260, tolerance mode; spp = 1..4 sample planes (BASELINE configs[2]: 4)
#ifndef FT_AO_EU
#define FT_AO_EU 7   // 72 VGPRs; 8 (64 VGPRs) was right before the cold copy of the pixel program existed: with it the allocator spills in the hot path (+40 %)
#endif
template <bool MULTI, int GEO>
__global__ __launch_bounds__(64 * FT_WAVES, FT_AO_EU) void kf_ao_temporal(AOTemporalArgs a)
{
    if (tile_order_rides<64 * FT_WAVES>(a.sort)) return;   // the trace kernel's next launch order, as extra grid rows (tile_order.h)
    const uint2 BLK = block_xy<0>();
    __shared__ uint32_t s_mask[FT_WAVES][4][18];
    __shared__ MaskRows s_rows[FT_WAVES];
    const int  lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // grid = (tile columns / FT_WAVES, tile rows): no integer division per wave
    const int  txr = BLK.x * FT_WAVES + wave;
    const bool tile_ok = txr < a.tiles_x;
    const int  tx = tile_ok ? txr : 0, ty = (int)BLK.y + a.tile_y0;
    const int  lx = lane & 7, ly = lane >> 3;
    const int  x = tx * 8 + lx, y = ty * 8 + ly;
    const bool in_image = tile_ok && x < a.w && y < a.h && y >= a.y0 && y < a.y1;
    const bool edge     = tile_ok && (x >= a.w || y >= a.h);
    const uint32_t pix  = in_image ? (uint32_t)(y * a.w + x) : (uint32_t)(a.gb2.y0 * a.w);
    const float d_raw   = fm::ld<float>(a.depth.p, pix * 4u);
    const uint2 cg2_raw = fm::ld<uint2>(a.gb2.p, pix * 8u);
    const uint32_t cg3y_raw = fm::ld<uint32_t>(a.gb3.p, pix * 8u + 4u);
    build_mask_rows<true>(s_rows[wave], s_mask[wave], a.mask, MULTI ? a.spp : 1, a.mw, a.mh, tx, ty, a.y0, a.y1, lane, tile_ok);
    if (!tile_ok) return;
    // the pixel's program, run once — and a second time (cold copy) by a wave that noted a history tap on a knife edge: kf_shadows_temporal
    bool flag = false;
    auto pixel = [&](const float d_in, const uint2 cg2_in, const uint32_t cg3y_in, const bool redo) -> uint32_t {
        const float    d    = edge ? 0.0f : d_in;
        const uint2    cg2  = edge ? make_uint2(0u, 0u) : cg2_in;
        const uint32_t cg3y = edge ? 0u : cg3y_in;
        const bool     live = (in_image || edge) && d != 1.0f;
        Reproj<2, false, false, GEO> rp;
        rp.M = a.vpi; rp.pgb2 = a.pgb2.p; rp.pgb3 = a.pgb3.p; rp.pdepth = a.pdepth.p; rp.hist = a.hist.p; rp.hist_moments = nullptr; rp.hist_len = a.hist_len.p;
        rp.geo = a.geo_hist;
        rp.g = HistGeom { a.w, a.h, a.pgb2.y0, a.pgb2.y1 };
        uint32_t ovr = 0u, known = 0u;
        if (redo && live)   // see kf_shadows_temporal
        {
            rp.issue(x, y, d, cg2.y, fm::lo(cg3y), 0.0f, fm::oct_unit(cg2.x), mk3(0, 0, 0), nullptr, 0.0f);
            ReprojOut r0;
            rp.template resolve<true>(r0);
            if (rp.near13)
            {
                known = rp.near13;
                ovr   = rp.exact_bits(known, x, y, d, cg2.x, cg2.y);
                if ((((ovr ^ rp.valid13) & known) & 0xfu) != 0u)
                {
                    const uint32_t rest = 0x1ff0u & ~known;
                    ovr |= rp.exact_bits(rest, x, y, d, cg2.x, cg2.y);
                    known |= rest;
                }
            }
        }
        if (live) rp.issue(x, y, d, cg2.y, fm::lo(cg3y), 0.0f, fm::oct_unit(cg2.x), mk3(0, 0, 0), nullptr, 0.0f);
        if (!redo && a.apron_flag && __ballot(live && in_image && y >= a.band_y0 && y < a.band_y1 && rp.apron_miss) && lane == 0) atomicOr(a.apron_flag, 1u);
        int sum, own;
        mask_window<MULTI>(s_rows[wave], lx, ly, sum, own);   // popcounts while the history loads are in flight
        const float mean = fm::div_by_inrange((float)sum, div_prepare(289.0f * (float)a.spp));
        flag = false;
        rp.near13 = 0u;
        if (in_image || edge)
        {
            float out = 1.0f, hlen = 0.0f;
            if (live)
            {
                const float ao = fm::div_by_inrange((float)own, div_prepare((float)a.spp));
                ReprojOut   r;
                const bool  success = rp.template resolve<true>(r, ovr, known);
                hlen = fm::fmin_(32.0f, success ? r.length + 1.0f : 1.0f);
                float hao = r.col[0];
                if (success)
                {
                    const float sd = fm::sqrt1(fm::fmax_(fm::var_rn(mean, mean), 0.0f));
                    hao = fm::fmin_(fm::fmax_(hao, mean - 0.5f * sd), mean + 0.5f * sd);
                }
                const float al = success ? fm::fmax_(a.alpha, fm::rcp_nr(hlen)) : 1.0f;
                out = fm::mix_rn(hao, ao, al);
            }
            if (in_image)
            {
                *reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.out) + pix * 2u)     = fm::half_bits(out);
                *reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.out_len) + pix * 2u) = fm::half_bits(hlen);
                // next frame's reprojection record: this pixel's oct normal, mesh id and AO value (copies of what the images hold)
                if (a.geo_out) *reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.geo_out) + pix * 8u) = make_uint2(cg2.x, (cg3y & 0xffffu) | ((uint32_t)fm::half_bits(out) << 16));
            }
            flag = out < 1.0f;
        }
        return live ? rp.near13 : 0u;
    };
    const uint32_t doubt = pixel(d_raw, cg2_raw, cg3y_raw, false);
    if (__any(doubt != 0u))   // rare: the cold copy (re-reads the centre texels: nothing of the first run is kept)
        pixel(fm::ld<float>(a.depth.p, pix * 4u), fm::ld<uint2>(a.gb2.p, pix * 8u), fm::ld<uint32_t>(a.gb3.p, pix * 8u + 4u), true);
    const unsigned long long any = __ballot(flag);
    if (lane == 0) a.tile_class[(size_t)ty * a.tiles_x + tx] = any ? 1 : 0;
}


// ------------------------------------------------------------------------------------------------------------------------
// ao_denoise_bilateral_blur.comp:75-139, tolerance mode.  LDS-tiled: the tile + its apron along the blur direction is decoded
// ONCE (linear eye depth, unit normal, AO value: 20 B per texel in LDS) instead of per tap — 8 taps of a radius-4 blur re-derived
// an octahedral decode + a normalisation + a reciprocal each.  The staging step and the 1-D tap loop are atrous_filters.h.
template <int RADIUS>
__global__ __launch_bounds__(256) void kf_ao_blur(AOBlurArgs a)
{
    const uint2 BLK = block_xy<0>();
    constexpr int kMaxTexels = 32 * (8 + 2 * RADIUS);   // the vertical pass is the larger footprint
    __shared__ float4 s_nz[kMaxTexels];                 // unit normal, linear eye depth
    __shared__ float  s_ao[kMaxTexels];
    __shared__ float  s_gauss[2 * RADIUS + 1];
    const int SW = 32 + 2 * RADIUS * a.dx, SH = 8 + 2 * RADIUS * a.dy;
    const int ox = (int)BLK.x * 32 - RADIUS * a.dx, oy = a.y0 + (int)BLK.y * 8 - RADIUS * a.dy;
    // the centre's own reads (tile class, depth) travel with the staging loads: one memory round trip before the barrier
    const int  lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int  x = (int)BLK.x * 32 + lx, y = a.y0 + (int)BLK.y * 8 + ly;
    const bool have = x < a.w && y < a.y1;
    const uint32_t o = have ? (uint32_t)(y * a.w + x) : (uint32_t)(a.y0 * a.w);
    const uint8_t  tclass = a.tile_class[have ? (size_t)(y >> 3) * a.tiles_x + (x >> 3) : 0];
    const float    cdepth = fm::ld<float>(a.depth.p, o * 4u);
    if ((int)threadIdx.x <= 2 * RADIUS) s_gauss[threadIdx.x] = gaussian_weight_fast((float)((int)threadIdx.x - RADIUS), (float)RADIUS * (1.0f / 1.5f));
    for (int i = threadIdx.x; i < SW * SH; i += 256)
    {
        const int  sy = i / SW, sx = i - sy * SW;
        ao_stage_texel(a, ox + sx, oy + sy, s_nz[i], s_ao[i], [](bool, int, int, float) {});
    }
    __syncthreads();
    if (!have) return;
    uint16_t* outp = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.out) + o * 2u);
    const uint16_t one = 0x3c00u;
    if (!tclass) { *outp = one; return; }   // cleared image (ray_traced_ao.cpp:1048-1055)
    if (cdepth == 1.0f) { *outp = one; return; }
    const int ci = (ly + RADIUS * a.dy) * SW + lx + RADIUS * a.dx, stride = a.dy * SW + a.dx;
    const float4 c  = s_nz[ci];
    float total_ao = s_ao[ci], total_w = 1.0f;
#pragma unroll
    for (int i = -RADIUS; i <= RADIUS; i++)
    {
        if (i == 0) continue;
        const float4 t  = s_nz[ci + i * stride];
        const float  w  = ao_tap_weight(&s_gauss[i + RADIUS], c.w, t.w, c.x * t.x + c.y * t.y + c.z * t.z);
        total_ao += w * s_ao[ci + i * stride];
        total_w += w;
    }
    *outp = fm::half_bits(ao_normalise(total_ao, total_w));
}

// Both passes of the separable blur in ONE launch: the X result of the tile's rows + a RADIUS-row apron above
// and below never leaves LDS.  Per 32 x TH output tile: (32 + 2R) x (TH + 2R) input texels are fetched and decoded once (the
// two-launch form fetched the tile + apron twice and wrote / re-read the X image: 2 x 74 MB of counter traffic at 1080p for 33 MB of
// algorithmic bytes), the X pass runs on 32 x (TH + 2R) texels, the Y pass on 32 x TH.  The X result is rounded to fp16 exactly as
// the R16F blur image stored it, tile classes / sky texels / out-of-band rows follow the same rules texel by texel, so the output
// is BIT-IDENTICAL to kf_ao_blur run twice (tests/test_gpu_fused.py); IMG_BLUR0 is not written in this form.
#ifndef FT_AO_BLUR_ROWS
#define FT_AO_BLUR_ROWS 1      // block_map.h block_xy<R>: tile rows per XCD run for the fused AO blur (0: identity, then HR_COLS8 bit 8 applies)
#endif
template <int RADIUS, int TH>
__global__ __launch_bounds__(256) void kf_ao_blur_xy(AOBlurArgs a)
{
    const uint2 BLK = block_xy<FT_AO_BLUR_ROWS>();
    if ((int)BLK.x * 32 >= a.w) return;   // a padding column of the launch (block_map.h grid_cols)
    constexpr int SW = 32 + 2 * RADIUS, SH = TH + 2 * RADIUS;
    __shared__ float4  s_nz[SH * SW];      // unit normal, linear eye depth
    __shared__ float   s_ao[SH * SW];
    __shared__ uint8_t s_kind[SH * SW];    // 0: not resident (reads as zeros), 1: cleared tile or sky (1.0), 2: filtered
    __shared__ float   s_x[SH * 32];       // X pass, as the R16F image would hold it
    __shared__ float   s_gauss[2 * RADIUS + 1];
    const int bx0 = (int)BLK.x * 32, by0 = a.y0 + (int)BLK.y * TH;
    const int ox = bx0 - RADIUS, oy = by0 - RADIUS;
    if ((int)threadIdx.x <= 2 * RADIUS) s_gauss[threadIdx.x] = gaussian_weight_fast((float)((int)threadIdx.x - RADIUS), (float)RADIUS * (1.0f / 1.5f));
    for (int i = threadIdx.x; i < SW * SH; i += 256)
    {
        const int  sy = i / SW, sx = i - sy * SW;
        ao_stage_texel(a, ox + sx, oy + sy, s_nz[i], s_ao[i], [&](bool ok, int px, int py, float z) {
            const uint8_t tc = a.tile_class[ok ? (size_t)(py >> 3) * a.tiles_x + (px >> 3) : 0];
            s_kind[i] = !ok ? 0 : ((!tc || z == 1.0f) ? 1 : 2);
        });
    }
    __syncthreads();
    // X pass over the tile's columns and SH rows
    for (int j = threadIdx.x; j < SH * 32; j += 256)
    {
        const int sy = j >> 5, sx = j & 31, ci = sy * SW + sx + RADIUS;
        const uint8_t kind = s_kind[ci];
        float r = kind == 1 ? 1.0f : 0.0f;
        if (kind == 2) r = (float)__builtin_bit_cast(_Float16, fm::half_bits(ao_blur_1d<RADIUS>(s_nz, ci, 1, s_ao, ci, 1, s_gauss)));
        s_x[j] = r;
    }
    __syncthreads();
    // Y pass over the tile
    for (int j = threadIdx.x; j < TH * 32; j += 256)
    {
        const int ly = j >> 5, lx = j & 31, x = bx0 + lx, y = by0 + ly;
        if (x >= a.w || y >= a.y1) continue;
        uint16_t* outp = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.out) + (uint32_t)(y * a.w + x) * 2u);
        const int ci = (ly + RADIUS) * SW + lx + RADIUS, xi = (ly + RADIUS) * 32 + lx;
        if (s_kind[ci] != 2) { *outp = 0x3c00u; continue; }   // cleared image (ray_traced_ao.cpp:1048-1055) / sky
        *outp = fm::half_bits(ao_blur_1d<RADIUS>(s_nz, ci, SW, s_x, xi, 32, s_gauss));
    }
}

// run-time radius: plain gathers
__global__ __launch_bounds__(256) void kf_ao_blur_generic(AOBlurArgs a)
{
    const uint2 BLK = block_xy<0>();
    __shared__ float s_gauss[2 * 32 + 1];
    if ((int)threadIdx.x <= 2 * a.radius) s_gauss[threadIdx.x] = gaussian_weight_fast((float)((int)threadIdx.x - a.radius), (float)a.radius * (1.0f / 1.5f));
    __syncthreads();
    const int x = BLK.x * 32 + (threadIdx.x & 31), y = a.y0 + BLK.y * 8 + (threadIdx.x >> 5);
    if (x >= a.w || y >= a.y1) return;
    const uint32_t o = (uint32_t)(y * a.w + x);
    uint16_t* outp = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.out) + o * 2u);
    const uint16_t one = 0x3c00u;
    if (!a.tile_class[(size_t)(y >> 3) * a.tiles_x + (x >> 3)]) { *outp = one; return; }
    const float d = fm::ld<float>(a.depth.p, o * 4u);
    if (d == 1.0f) { *outp = one; return; }
    const float cd = fm::rcp_nr(fm::mad_rn(a.zbp[2], d, a.zbp[3]));
    const f3    cn = fm::oct_unit(fm::ld<uint32_t>(a.gb2.p, o * 8u));
    float total_ao = (float)__builtin_bit_cast(_Float16, fm::ld<uint16_t>(a.in.p, o * 2u)), total_w = 1.0f;
    for (int i = -a.radius; i <= a.radius; i++)
    {
        if (i == 0) continue;
        const int  px = x + a.dx * i, py = y + a.dy * i;
        const bool ok = !(px < 0 || py < a.y0 || px >= a.w || py >= a.y1);
        const uint32_t off = ok ? (uint32_t)(py * a.w + px) : o;
        float    z  = fm::ld<float>(a.depth.p, off * 4u);
        uint32_t g2 = fm::ld<uint32_t>(a.gb2.p, off * 8u);
        uint16_t v  = fm::ld<uint16_t>(a.in.p, off * 2u);
        if (!ok) { z = 0.0f; g2 = 0u; v = 0; }
        const float sd = fm::rcp_nr(fm::mad_rn(a.zbp[2], z, a.zbp[3]));
        const float w  = ao_tap_weight(&s_gauss[i + a.radius], cd, sd, fm::dot(cn, fm::oct_unit(g2)));
        total_ao += w * (float)__builtin_bit_cast(_Float16, v);
        total_w += w;
    }
    *outp = fm::half_bits(ao_normalise(total_ao, total_w));
}

} // namespace

namespace hr {

void launch_ao_temporal_fast(const AOTemporalArgs& a_, int n_tiles, hipStream_t st)
{
    AOTemporalArgs a = a_;
    const dim3 grid = grid_with_sort(a.sort, grid_cols(cdiv(a.tiles_x, FT_WAVES), 5), a.tiles_y);
    if (a.geo_hist && a.geo_band)
    {
        if (a.spp > 1) hipLaunchKernelGGL((kf_ao_temporal<true, 1>), grid, dim3(64 * FT_WAVES), 0, st, a);
        else hipLaunchKernelGGL((kf_ao_temporal<false, 1>), grid, dim3(64 * FT_WAVES), 0, st, a);
    }
    else if (a.geo_hist)
    {
        if (a.spp > 1) hipLaunchKernelGGL((kf_ao_temporal<true, 2>), grid, dim3(64 * FT_WAVES), 0, st, a);
        else hipLaunchKernelGGL((kf_ao_temporal<false, 2>), grid, dim3(64 * FT_WAVES), 0, st, a);
    }
    else if (a.spp > 1) hipLaunchKernelGGL((kf_ao_temporal<true, 0>), grid, dim3(64 * FT_WAVES), 0, st, a);
    else hipLaunchKernelGGL((kf_ao_temporal<false, 0>), grid, dim3(64 * FT_WAVES), 0, st, a);
}

void launch_ao_blur_fast(const AOBlurArgs& a, hipStream_t st)
{
    const dim3 grid(cdiv(a.w, 32), cdiv(a.y1 - a.y0, 8));
    if (a.radius == 4) hipLaunchKernelGGL(kf_ao_blur<4>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(kf_ao_blur_generic, grid, dim3(256), 0, st, a);
}

#ifndef FT_AO_BLUR_TH
#define FT_AO_BLUR_TH 16   // tile height: 16 against 8 -> 24.8 against 26.5 us; 16 against 32 -> 1080p 23.5 against 25.7 us, 4K 66.5 against 70.5 (32: 1.56x instead of 1.88x apron reads, but 38.7 KB of LDS per workgroup)
#endif
bool launch_ao_blur_xy_fast(const AOBlurArgs& a, hipStream_t st)
{
    if (a.radius != 4) return false;   // other radii keep the two-launch form
    hipLaunchKernelGGL((kf_ao_blur_xy<4, FT_AO_BLUR_TH>), dim3(grid_cols(cdiv(a.w, 32), 8), cdiv(a.y1 - a.y0, FT_AO_BLUR_TH)), dim3(256), 0, st, a);
    return true;
}

} // namespace hr
