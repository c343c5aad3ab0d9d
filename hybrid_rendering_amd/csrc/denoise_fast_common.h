// What the tolerance-mode ("fast") denoise / resolve units share: hr_*_params.exact == 0.  One unit per pass —
// denoise_fast_shadows.hip, denoise_fast_ao.hip, denoise_fast_reflections.hip, denoise_fast_resolve.hip — each includes this header
// FIRST and holds only its own kernels, knobs and launchers.
//
// Same stages, inputs, outputs and tile-classification rules as the exact kernels in shadows.hip / ao.hip / reflections.hip /
// ddgi.hip / upsample.h (which stay the bit-for-bit parity mode), restructured for the hardware instead of for the order of
// operations of the GLSL:
//   * arithmetic through fast_math.h (v_rcp / v_rsq / v_sqrt / v_exp / v_log, contracted FMAs);
//   * reprojection: the view-projection-inverse products shared by the taps are hoisted (M * (u, v, d, 1) is affine in d), the
//     previous-frame normal is compared un-normalised (cos^2 > 0.1 <=> dot^2 > 0.1 |n|^2), one validity / address computation per
//     tap serves all history images, and only the bytes of a texel that are used are loaded;
//   * 17x17 neighbourhood statistics: packed visibility masks are bit-sliced across the spp planes and popcounted with
//     v_bfe + v_bcnt (accumulating); the reflections' colour statistics are separable sums staged through LDS;
//   * a-trous / bilateral blur: step-specialised, interior tiles skip every bounds test, AO blur stages decoded normals and
//     linear depth of the tile + apron in LDS once instead of re-deriving them per tap;
//   * DDGI probe-grid sample: the octahedral coordinates of the surface normal are computed once, not per probe.
// Validated against the oracle within the stated tolerance by tests/test_gpu_tolerance.py; masks and ray counts do not pass
// through these units.
#pragma once
#include "hr_internal.h"
#include "pass_args.h"
#include "fast_math.h"
#include "block_map.h"
#include "exact_predicates.h"   // before any contract(fast): the knife-edge fallbacks keep the parity kernels' arithmetic

#pragma clang fp contract(fast)

#ifndef HR_TAP_BAND
#define HR_TAP_BAND 0.4f   // scale of the guard bands of Reproj::tap_valid (developer A/B; 0: never in doubt, the cold copy stays compiled in).  Measured at 1080p, shadows temporal: 0 -> +0 %, 0.3 -> +2.4 %, 1.0 -> +8 % (how often a wave runs twice); 0.4 keeps >= 3x the error bound of the fast operands
#endif

using namespace hr;

#include "atrous_filters.h"   // the a-trous / blur filter bodies; under the contract(fast) above, like the kernels that call them

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// reprojection.glsl:115-328, tolerance-mode restatement
struct HistGeom { int w, h, y0, y1; };   // every history / previous-G-buffer image of a pass shares one geometry

struct ReprojOut { float col[3]; float mom[2]; float length; };

// HIST_BPP: bytes per texel of the colour history — 2 (AO, R16F), 4 (shadows, RG16F: .r), 8 (reflections, RGBA16F: .rgb).
// Two phases so that a kernel can put independent work (mask popcounts, LDS passes) between them:
//   issue()    history coordinates + all 21 loads of the 2x2 bilinear footprint and the history-length texel — nothing is waited for;
//   resolve()  validity tests, weighting, normalisation (+ the rare 3x3 fallback with its own loads).
// GEO: where the previous frame's geometry comes from.  false: the caller's previous G-buffer — oct normal from GB2 (.x word of an
// 8-byte texel), mesh id from GB3 (.y word), i.e. two images of which half of every cache line is used.  true: the pass's own
// 8-byte geometry record {oct normal, mesh id | linear z} that its temporal kernel wrote LAST frame (it writes one anyway, for the
// a-trous taps; the two halves of the buffer alternate), and — with MOMENTS — the history length comes out of the 8-byte moments texel of
// the nearest tap, which is always one of the four bilinear taps: 4 images, 16 loads, every line fully used, against 5 images and 21
// loads.  Same values (the record holds copies of the G-buffer words), so the results are bit-identical.  GEO = 1: as described
// (shadows, reflections).  GEO = 2 (AO, whose history value is a single fp16): the record is {oct normal, mesh id | AO history}, i.e. the
// colour history rides in the record too — 2 images + the history length, 9 loads against 17.
// PATHS (TemporalPaths bits; shadows on the record path, GEO = 1): TP_PAIRS — the taps (bx, py) and (bx + 1, py) of a footprint row are
// neighbours in memory, so one load per image and row fetches both: 8 loads for 16, the same bytes; see issue().
template <int HIST_BPP, bool MOMENTS, bool REFL, int GEO = 0, int PATHS = 0>
struct Reproj
{
    static constexpr bool PAIRS   = (PATHS & TP_PAIRS) != 0 && GEO == 1 && MOMENTS && HIST_BPP == 4;
    struct alignas(8) Pair8 { uint32_t x0, y0, x1, y1; };   // two 8-byte texels
    struct alignas(4) Pair4 { uint32_t v0, v1; };           // two 4-byte texels
    static constexpr int NC = HIST_BPP == 8 ? 3 : 1;
    const float* __restrict__ M;
    const void* __restrict__  pgb2;
    const void* __restrict__  pgb3;
    const void* __restrict__  pdepth;
    const void* __restrict__  hist;
    const void* __restrict__  hist_moments;
    const void* __restrict__  hist_len;
    const void* __restrict__  geo;          // GEO: previous frame's {oct normal, mesh id | linear z} records
    HistGeom   g;
    f3         cur_pos, cur_n;
    float      cur_id, hfx, hfy, band;
    uint32_t   near13;       // resolve<NOTE>: bit s (< 4) = bilinear tap s on a knife edge, bit 4 + k = tap k of the 3x3 fallback
    uint32_t   valid13;      // resolve<NOTE>: the verdicts used (same layout); bit 13 = the 3x3 fallback was evaluated
    int        hcx, hcy;
    bool       inb, lok, tok[4], apron_miss;   // apron_miss: the footprint touched an image row that is not resident (row bands)
    fm::Unproj hb;
    uint32_t   g2x[4], g3y[4], mm[4], hx[4], hy[4], lraw;
    uint32_t   mlen[4];
    float      td[4];

    // texel (px, py) of the previous frame passes is_reprojection_valid (reprojection.glsl:52-67) for this pixel; branch-free.
    // NOTE (shadows / AO): `near` = the tap sits inside a guard band around one of the two thresholds, where the fast operands cannot be
    // trusted with the decision (they are good to ~3 ulp of the positions' coordinates; the parity kernels round every operation):
    // |plane distance - 5| < band = HR_TAP_BAND (1e-4 + 3e-6 |p|_1) (cur_pos and the tap's position are each good to ~3 ulp of their
    // coordinates, their difference along the normal to ~4e-7 |p|_1), |cos^2 - 0.1 |n'|^2| <= HR_TAP_BAND 4e-6 |n'|^2 (fast: ~1e-7).  Branch-free, 4 VALU per tap.  The bands decide how often a wave runs its pixels twice
    // (first version, 0.01 + 1.6e-5 |p|_1 and 4e-4: shadows temporal +18 %, AO +15 % at 1080p; docs/EXPERIMENTS.md R5.1).
    template <bool NOTE>
    HR_DEV bool tap_valid(uint32_t q2x, uint32_t q3y, float d, bool& near) const
    {
        const f3    hn = fm::oct_raw(q2x);
        const float dn = fm::dot(cur_n, hn), hh = fm::dot(hn, hn);
        const f3    hp = fm::unproject_at(hb, M, d);
        const float pd = __builtin_fabsf(fm::dot(sub3(cur_pos, hp), cur_n));
        const float t  = dn * dn - 0.1f * hh;
        const int   pre = (int)inb & (int)(cur_id == fm::lo(q3y));
        near = false;
        if constexpr (NOTE) near = (pre & ((int)(__builtin_fabsf(pd - 5.0f) < band) | (int)(__builtin_fabsf(t) <= (HR_TAP_BAND * 4e-6f) * hh))) != 0;
        return (pre & (int)!(pd > 5.0f) & (int)(t > 0.0f)) != 0;
    }
    HR_DEV uint32_t tap_offset(int px, int py, bool& ok) const
    {
        ok = ((int)(px < 0) | (int)(py < g.y0) | (int)(px >= g.w) | (int)(py >= g.y1)) == 0;
        return ok ? (uint32_t)(py * g.w + px) : (uint32_t)(g.y0 * g.w);
    }
    HR_DEV void hist_decode(uint32_t rx, uint32_t ry, float* c) const
    {
        if constexpr (HIST_BPP == 2) c[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)rx);
        else if constexpr (HIST_BPP == 4) c[0] = fm::lo(rx);
        else { c[0] = fm::lo(rx); c[1] = fm::hi(rx); c[2] = fm::lo(ry); }
    }
    HR_DEV void hist_load(uint32_t off, uint32_t& rx, uint32_t& ry) const
    {
        ry = 0u;
        if constexpr (HIST_BPP == 2) rx = fm::ld<uint16_t>(hist, off * 2u);
        else if constexpr (HIST_BPP == 4) rx = fm::ld<uint32_t>(hist, off * 4u);
        else { const uint2 t = fm::ld<uint2>(hist, off * 8u); rx = t.x; ry = t.y; }
    }

    HR_DEV void issue(int x, int y, float depth, uint32_t c2y, float cur_id_, float curvature, f3 cur_n_, f3 cam_pos, const float* __restrict__ prev_vp, float ray_length)
    {
        cur_id = cur_id_; cur_n = cur_n_;
        const float fw = (float)g.w, fh = (float)g.h;
        // (x + 0.5) / w correctly rounded (round 5): the clip -> world products below cancel 3-4 digits, so ONE ulp of tu moved a world
        // position by up to ~1e-3 — 20 ulp of its coordinates — and the plane distance of a history tap with it (measured: the guard band of
        // tap_valid had to be 10x wider than the error of everything else).  With the parity kernels' tu / tv the products are theirs
        // bit for bit (same operation order, fast_math.h) and only the perspective divide differs (rcp_nr: ~1 ulp).  ~10 VALU per pixel.
        const float tu = fm::div_by_inrange((float)x + 0.5f, div_prepare(fw)), tv = fm::div_by_inrange((float)y + 0.5f, div_prepare(fh));
        const float mvx = fm::lo(c2y), mvy = fm::hi(c2y);
        cur_pos = fm::unproject_at(fm::unproject_base(M, tu, tv), M, depth);
        band    = HR_TAP_BAND * 1e-4f + (HR_TAP_BAND * 3e-6f) * (__builtin_fabsf(cur_pos.x) + __builtin_fabsf(cur_pos.y) + __builtin_fabsf(cur_pos.z));   // tap_valid<true>
        hfx = (float)x + mvx * fw; hfy = (float)y + mvy * fh;   // mv (fp16) * extent (<= 2^12) is exact: same texel as the exact mode
        if (REFL)
        {
            if (ray_length > 0.0f && curvature == 0.0f)
            {
                // virtual_point_reprojection (reprojection.glsl:71-111) with the parity kernels' operations (exact_predicates.h: the weights of the
                // history taps — and so the interpolated moments — are then the oracle's; round 5, late)
                exact::virtual_point(M, prev_vp, cam_pos, x, y, g.w, g.h, depth, ray_length, hfx, hfy);
            }
            hcx = (int)hfx; hcy = (int)hfy;
        }
        else
        {
            hcx = (int)(hfx + 0.5f);
            hcy = (int)(hfy + 0.5f);
        }
        inb = ((int)(hcx < 0) | (int)(hcy < 0) | (int)(hcx > g.w - 1) | (int)(hcy > g.h - 1)) == 0;
        hb  = fm::unproject_base(M, tu + mvx, tv + mvy);
        // an outside tap loads a resident address (its value is discarded in resolve()), so no load sits behind a branch
        const int bx = (int)hfx, by = (int)hfy;
        apron_miss = ((unsigned)by < (unsigned)g.h && (by < g.y0 || by >= g.y1)) || ((unsigned)(by + 1) < (unsigned)g.h && (by + 1 < g.y0 || by + 1 >= g.y1));
        uint32_t  off[4];
#pragma unroll
        for (int s = 0; s < 4; s++) off[s] = tap_offset(bx + (s & 1), by + (s >> 1), tok[s]);
        const uint32_t loff = tap_offset(hcx, hcy, lok);
        if constexpr (PAIRS)
        {
            // Both taps of a row from the texel pair at column bxc = bx clamped into [0, w - 2] (the launcher grants w >= 2), so the pair never
            // leaves its row; a row that is not resident reads row y0, as a lone tap does.  bx == bxc: the taps are the pair.  bx < bxc (bx < 0):
            // tap 0 is outside the image (tok: its value is discarded) and tap 1, if inside, is the pair's first texel.  bx > bxc: tap 0, if
            // inside, is the pair's second texel and tap 1 is outside.
            const int  bxc = bx < 0 ? 0 : (bx > g.w - 2 ? g.w - 2 : bx);
            const bool up = bx > bxc, down = bx < bxc;
            lraw = 0u;
#pragma unroll
            for (int r = 0; r < 2; r++)
            {
                const int      py = by + r;
                const uint32_t o  = (uint32_t)(((py >= g.y0 && py < g.y1) ? py : g.y0) * g.w + bxc);
                const Pair8 q = fm::ld<Pair8>(geo, o * 8u), m = fm::ld<Pair8>(hist_moments, o * 8u);
                const Pair4 d = fm::ld<Pair4>(pdepth, o * 4u), c = fm::ld<Pair4>(hist, o * 4u);
                const int   s0 = 2 * r, s1 = 2 * r + 1;
                g2x[s0] = up ? q.x1 : q.x0;  g3y[s0] = up ? q.y1 : q.y0;  td[s0] = __builtin_bit_cast(float, up ? d.v1 : d.v0);  hx[s0] = up ? c.v1 : c.v0;
                mm[s0]  = up ? m.x1 : m.x0;  hy[s0] = 0u;
                g2x[s1] = down ? q.x0 : q.x1; g3y[s1] = down ? q.y0 : q.y1; td[s1] = __builtin_bit_cast(float, down ? d.v0 : d.v1); hx[s1] = down ? c.v0 : c.v1;
                mm[s1]  = down ? m.x0 : m.x1; hy[s1] = 0u;
                // the nearest history texel (hcx, hcy) is one of the four taps (below): its length word, picked here so that four of them need not live on
                if (hcy - by == r) lraw = (hcx - bx) != 0 ? (down ? m.y0 : m.y1) : (up ? m.y1 : m.y0);
            }
        }
        else
        {
#pragma unroll
            for (int s = 0; s < 4; s++)
            {
                if constexpr (GEO != 0)
                {
                    const uint2 q = fm::ld<uint2>(geo, off[s] * 8u);
                    g2x[s] = q.x; g3y[s] = q.y;
                }
                else
                {
                    g2x[s] = fm::ld<uint32_t>(pgb2, off[s] * 8u);
                    g3y[s] = fm::ld<uint32_t>(pgb3, off[s] * 8u + 4u);
                }
                td[s]  = fm::ld<float>(pdepth, off[s] * 4u);
                if constexpr (GEO == 2) { hx[s] = g3y[s] >> 16; hy[s] = 0u; }
                else hist_load(off[s], hx[s], hy[s]);
                if constexpr (MOMENTS && GEO != 0)
                {
                    const uint2 m = fm::ld<uint2>(hist_moments, off[s] * 8u);
                    mm[s] = m.x; mlen[s] = m.y;
                }
                else mm[s] = MOMENTS ? fm::ld<uint32_t>(hist_moments, off[s] * 8u) : 0u;
            }
        }
        if constexpr (PAIRS) {}
        else if constexpr (MOMENTS && GEO != 0)
        {
            // the nearest history texel (hcx, hcy) is one of the four taps: bx <= hcx <= bx + 1 (truncation on both sides)
            const int sel = (hcx - bx) + 2 * (hcy - by);
            lraw = sel == 0 ? mlen[0] : (sel == 1 ? mlen[1] : (sel == 2 ? mlen[2] : mlen[3]));
        }
        else if (MOMENTS) lraw = fm::ld<uint32_t>(hist_moments, loff * 8u + 4u);
        else lraw = fm::ld<uint16_t>(hist_len, loff * 2u);
    }

    // NOTE = true (shadows, AO): taps on a knife edge are recorded in near13.  `known` (bit layout of near13): taps whose validity is
    // taken from `ovr` — the parity kernels' verdicts of exact_bits() — instead of the fast test (and which are then not noted again).
    template <bool NOTE = false>
    HR_DEV bool resolve(ReprojOut& o, uint32_t ovr = 0u, uint32_t known = 0u)
    {
        const float fx = hfx - __builtin_floorf(hfx), fy = hfy - __builtin_floorf(hfy);
        const float wgt[4] = { (1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy };
        float sumw = 0.0f, col[NC], mom0 = 0.0f, mom1 = 0.0f;
        uint32_t noted = 0u, used = 0u;
#pragma unroll
        for (int c = 0; c < NC; c++) col[c] = 0.0f;
#pragma unroll
        for (int s = 0; s < 4; s++)
        {
            // an out-of-image texel reads as zeros (pinned rule) and is validated as such, as in the exact mode: its weight counts
            // in the normalisation, its (zero) values add nothing
            bool nr;
            bool v = tap_valid<NOTE>(tok[s] ? g2x[s] : 0u, tok[s] ? g3y[s] : 0u, tok[s] ? td[s] : 0.0f, nr);
            if (NOTE) { if ((known >> s) & 1u) v = (ovr >> s) & 1u; else noted |= (uint32_t)nr << s; used |= (uint32_t)v << s; }
            const float ws = v ? wgt[s] : 0.0f, wv = ((int)v & (int)tok[s]) ? wgt[s] : 0.0f;
            float c3[NC];
            hist_decode(hx[s], hy[s], c3);
#pragma unroll
            for (int c = 0; c < NC; c++) col[c] += wv * c3[c];
            // the moments keep the parity kernels' two roundings per term (no FMA): the variance downstream is m2 - m1^2, and where it is tiny
            // (<= 1e-8: a sixth of the surface texels of a young history) ONE fp32 ulp of a moment is a multiple of it — and the a-trous
            // chain divides luminance differences by its square root (docs/EXPERIMENTS.md R5.8)
            if (MOMENTS) { mom0 = fm::mad_rn(wv, fm::lo(mm[s]), mom0); mom1 = fm::mad_rn(wv, fm::hi(mm[s]), mom1); }
            sumw += ws;
        }
        // Normalisations are correctly rounded divisions (one shared denominator: fast_math.h div_by_inrange): a history of
        // all-equal values must come back EXACTLY (sum(w) v / sum(w) == v) — the tile classification tests `ao < 1`, `visibility > 0`
        bool valid = sumw >= 0.01f;
        if (valid)
        {
            const DivBy D = div_prepare(sumw);   // 0.01 <= sumw <= 1; numerators are fp16 values times weights <= 1
#pragma unroll
            for (int c = 0; c < NC; c++) col[c] = fm::div_by_inrange(col[c], D);
            if (MOMENTS) { mom0 = fm::div_by_inrange(mom0, D); mom1 = fm::div_by_inrange(mom1, D); }
        }
        else
        {
            // 3x3 fallback around the nearest history texel (:266-303); rare (disocclusion borders): kept rolled
            float cnt = 0.0f;
#pragma unroll
            for (int c = 0; c < NC; c++) col[c] = 0.0f;
            mom0 = mom1 = 0.0f;
#pragma unroll 1
            for (int k = 0; k < 9; k++)
            {
                bool           ok;
                const uint32_t qo = tap_offset(hcx + k % 3 - 1, hcy + k / 3 - 1, ok);
                uint32_t q2, q3;
                if constexpr (GEO != 0) { const uint2 q = fm::ld<uint2>(geo, qo * 8u); q2 = q.x; q3 = q.y; }
                else { q2 = fm::ld<uint32_t>(pgb2, qo * 8u); q3 = fm::ld<uint32_t>(pgb3, qo * 8u + 4u); }
                const float    qd = fm::ld<float>(pdepth, qo * 4u);
                uint32_t       qx, qy;
                if constexpr (GEO == 2) { qx = q3 >> 16; qy = 0u; }
                else hist_load(qo, qx, qy);
                const uint32_t qm = MOMENTS ? fm::ld<uint32_t>(hist_moments, qo * 8u) : 0u;
                bool nr;
                bool tv = tap_valid<NOTE>(ok ? q2 : 0u, ok ? q3 : 0u, ok ? qd : 0.0f, nr);
                if (NOTE) { if ((known >> (4 + k)) & 1u) tv = (ovr >> (4 + k)) & 1u; else noted |= (uint32_t)nr << (4 + k); used |= ((uint32_t)tv << (4 + k)) | (1u << 13); }
                if (tv)
                {
                    float c3[NC];
                    hist_decode(ok ? qx : 0u, ok ? qy : 0u, c3);
#pragma unroll
                    for (int c = 0; c < NC; c++) col[c] += c3[c];
                    if (MOMENTS) { mom0 += fm::lo(ok ? qm : 0u); mom1 += fm::hi(ok ? qm : 0u); }
                    cnt += 1.0f;
                }
            }
            if (cnt > 0.0f)
            {
                valid = true;
                const DivBy D = div_prepare(cnt);
#pragma unroll
                for (int c = 0; c < NC; c++) col[c] = fm::div_by_inrange(col[c], D);
                if (MOMENTS) { mom0 = fm::div_by_inrange(mom0, D); mom1 = fm::div_by_inrange(mom1, D); }
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++) o.col[c] = valid ? col[c] : 0.0f;
        o.mom[0] = valid ? mom0 : 0.0f;
        o.mom[1] = valid ? mom1 : 0.0f;
        o.length = ((int)valid & (int)lok) ? fm::lo(lraw) : 0.0f;
        near13 = noted; valid13 = used;
        return valid;
    }

    // The parity kernels' verdicts on the taps `which` of this pixel (bit layout of near13): their geometry is fetched again here (nothing of
    // the hot path stays live across this), every verdict is exact::tap_valid.  Runs for the few waves that noted a tap on a knife edge.
    // (x, y), depth, c2x, c2y: the pixel, its depth and its GB2 words as given to issue().
    HR_DEV uint32_t exact_bits(uint32_t which, int x, int y, float depth, uint32_t c2x, uint32_t c2y) const
    {
        const int bx = (int)hfx, by = (int)hfy;
        uint32_t  bits = 0u;
#pragma unroll 1
        while (which)
        {
            const int k = __builtin_ctz(which);
            which &= which - 1u;
            const int px = k < 4 ? bx + (k & 1) : hcx + (k - 4) % 3 - 1, py = k < 4 ? by + (k >> 1) : hcy + (k - 4) / 3 - 1;
            bool           ok;
            const uint32_t qo = tap_offset(px, py, ok);
            uint32_t q2, q3;
            if constexpr (GEO != 0) { const uint2 q = fm::ld<uint2>(geo, qo * 8u); q2 = q.x; q3 = q.y; }
            else { q2 = fm::ld<uint32_t>(pgb2, qo * 8u); q3 = fm::ld<uint32_t>(pgb3, qo * 8u + 4u); }
            const float qd = fm::ld<float>(pdepth, qo * 4u);
            bits |= (uint32_t)exact::tap_valid(M, x, y, g.w, g.h, depth, c2x, c2y, cur_id, hcx, hcy, ok ? q2 : 0u, ok ? q3 : 0u, ok ? qd : 0.0f) << k;
        }
        return bits;
    }
};

// at the top of a temporal kernel whose argument block carries a GeoApronArgs: true = this workgroup was one of the apron's (pass_args.h)
template <int THREADS>
HR_DEV bool geo_apron_rides(const GeoApronArgs& g)
{
    if (g.row0 < 0 || (int)blockIdx.y < g.row0) return false;
    const int      na = g.a1 - g.a0, total = (na + (g.b1 - g.b0)) * g.w;
    const int      stride = (int)(gridDim.y - (unsigned)g.row0) * (int)gridDim.x * THREADS;
    for (int i = (((int)blockIdx.y - g.row0) * (int)gridDim.x + (int)blockIdx.x) * THREADS + (int)threadIdx.x; i < total; i += stride)
    {
        const int      r = i / g.w, x = i - r * g.w, y = r < na ? g.a0 + r : g.b0 + (r - na);
        const uint32_t o = (uint32_t)(y * g.w + x);
        *reinterpret_cast<uint2*>(reinterpret_cast<char*>(g.out) + o * 8u) = make_uint2(fm::ld<uint32_t>(g.gb2, o * 8u), fm::ld<uint32_t>(g.gb3, o * 8u + 4u));
    }
    return true;
}

#define FT_WAVES 4   // waves (8x8 tiles) per workgroup of the shadows' and the AO temporal kernels
template <bool B> struct BoolC { static constexpr bool value = B; };

} // namespace

namespace hr {

// a riding sort (TileOrder::ride) goes behind the `rows` grid rows of a temporal launch of `grid_x` workgroups per row: the grid with it
static dim3 grid_with_sort(TileSortArgs& t, int grid_x, int rows)
{
    t.row0 = rows;
    return dim3(grid_x, rows + (t.groups ? cdiv(t.groups, grid_x) : 0));
}
// ... and the history apron's records (GeoApronArgs) behind the sort: ~4 texels per thread
static dim3 grid_with_apron(dim3 grid, GeoApronArgs& g, int threads)
{
    const int total = g.out ? ((g.a1 - g.a0) + (g.b1 - g.b0)) * g.w : 0;
    if (total <= 0) { g.row0 = -1; return grid; }
    g.row0 = (int)grid.y;
    return dim3(grid.x, grid.y + (unsigned)cdiv(total, (int)grid.x * threads * 4));
}

} // namespace hr
