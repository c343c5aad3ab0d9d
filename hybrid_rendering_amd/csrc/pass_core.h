// Host-side core of the three denoised passes (shadows.hip, ao.hip, reflections.hip): what a pass image's rows are, when the pass-owned
// geometry records may stand in for the caller's previous G-buffer, and the state and entry-point bodies the passes have in common.
// The first part is plain C++ over the public C header, so that a CPU program can compile and test it (tests/pass_core_check.cpp);
// PassCore, which owns device buffers, follows under __HIPCC__.
#pragma once
#include "../../include/hr_api.h"
#include <cstdint>
#include <string>

namespace hr {

// ------------------------------------------------------------------------------------------------ rows
// Which bands hr_*_create accepts.  There are two rules because the passes were published with two, and a caller's band that one of them
// accepts today must not start to fail (nor the other way round):
//   Shadows         checks the BAND: inside the image, band_y0 and band_y1 multiples of 8 (band_y1 == h may be ragged), halo >= 0 and a
//                   multiple of 8.  Without a band, band_y0 / band_y1 are the whole image.
//   AoReflections   checks only the RESIDENT rows it derives (band -/+ halo, clamped to the image): y0 and y1 multiples of 8 (y1 == h may be
//                   ragged).  So a band outside the image passes, and so does one whose rows and halo are no multiples of 8 but add up
//                   to one.  Without a band, band_y0 = band_y1 = 0.
enum class BandRule { Shadows, AoReflections };

struct PassRows
{
    int full_w = 0, full_h = 0, scale = 0;
    int w = 0, h = 0;                 // pass image: extent >> scale (the reference divides as float and truncates, ray_traced_shadows.cpp:80-83)
    int y0 = 0, y1 = 0;               // resident rows (band + halo)
    int band_y0 = 0, band_y1 = 0;
    int ry0 = 0, ry1 = 0;             // rows whose history / G-buffer may be read (band + history halo; AoReflections: the resident rows)
    int tiles_x = 0, tiles_y = 0;     // 8x8 tiles of the whole pass image
    int mw = 0, mh = 0;               // 8x4 mask words of the whole pass image

    // nullptr, or why the band is refused (the object is then not to be used)
    const char* init(int full_width, int full_height, int scale_, const hr_band* band, BandRule rule)
    {
        full_w = full_width; full_h = full_height; scale = scale_;
        w = full_width >> scale_; h = full_height >> scale_;
        y0 = 0; y1 = h; ry0 = 0; ry1 = h;
        band_y0 = 0; band_y1 = rule == BandRule::Shadows ? h : 0;
        if (band && band->band_y1 > band->band_y0)
        {
            if (rule == BandRule::Shadows && (band->band_y0 < 0 || band->band_y1 > h || (band->band_y0 & 7) || ((band->band_y1 & 7) && band->band_y1 != h) || band->halo < 0 || (band->halo & 7)))
                return "band rows must be multiples of 8 inside the pass image; halo a multiple of 8";
            band_y0 = band->band_y0; band_y1 = band->band_y1;
            y0 = band->band_y0 - band->halo < 0 ? 0 : band->band_y0 - band->halo;
            y1 = band->band_y1 + band->halo > h ? h : band->band_y1 + band->halo;
            ry0 = y0; ry1 = y1;
            if (rule == BandRule::AoReflections && ((y0 & 7) || ((y1 & 7) && y1 != h))) return "band rows must be multiples of 8";
            if (rule == BandRule::Shadows)
            {
                const int hh = band->history_halo > band->halo ? band->history_halo : band->halo;
                ry0 = band->band_y0 - hh < 0 ? 0 : band->band_y0 - hh;
                ry1 = band->band_y1 + hh > h ? h : band->band_y1 + hh;
            }
        }
        mw = (w + 7) / 8; mh = (h + 3) / 4;
        tiles_x = (w + 7) / 8; tiles_y = (h + 7) / 8;
        return nullptr;
    }
    // the tile grid of the resident rows: what the per-tile launches cover
    int  tile_y0() const { return y0 / 8; }
    int  resident_tiles_y() const { return (y1 + 7) / 8 - y0 / 8; }
    int  resident_tiles() const { return tiles_x * resident_tiles_y(); }
    bool banded() const { return y0 > 0 || y1 < h; }
};

// ------------------------------------------------------------------------------------------------ geometry records
// Tolerance mode: a pass's temporal kernel writes an 8-byte record per pixel — copies of the current G-buffer's words {oct normal, mesh id |
// linear z}; AO stores its own output in place of z — into one of two slots, which alternate, so last frame's records are still there when the
// next frame reprojects.  They stand for the caller's PREVIOUS G-buffer exactly when the caller hands back, as in->prev, the images it passed
// as in->cur in the previous call (the reference's ping-pong, g_buffer.cpp:208-211): then the reprojection reads them (shadows: 4 images, 16
// gathers per pixel, full cache lines; AO: 2 images + the history length, 9 gathers) instead of prev GB2 / GB3 (5 images, 21 / 17 gathers, half
// of every line unused), and this frame's a-trous taps read this frame's slot.  A previous G-buffer that ALIASES the current one (one buffer
// rewritten in place) is read as the caller passed it.  AO's record also holds its colour history, which is last frame's only if the caller
// alternated ping_pong: it passes the index, the other two pass -1.
// Where the slots live is the pass's business (shadows: the two halves of `nd`; AO, reflections: geo[2], allocated iff `history`).  Shadows
// writes records in every tolerance-mode frame, for its a-trous stages, so it advances with `history` off as well — a read slot then never
// appears; AO and reflections have no slots then and invalidate instead.
struct GeoRecords
{
    bool        history = true;    // developer A/B switch HR_GEO_HISTORY=0 (read once at create)
    bool        require = false;   // HR_DEBUG_REQUIRE_GEO (tests): a tolerance-mode temporal stage that had records and could not reproject from them fails
    bool        valid = false;     // slot `parity` holds the records of the last frame this pass rendered
    int         parity = 0, pp = -1;
    const void* gb2 = nullptr;     // in->cur.gb2 / gb3 of that frame
    const void* gb3 = nullptr;

    struct Step
    {
        int  read;                 // slot to reproject from, -1: the caller's previous G-buffer
        int  write;                // slot of this frame's records
        bool require_failed;
    };
    // reset_history, the parity mode (whose side images have another layout), no slots allocated
    void invalidate() { valid = false; }
    Step advance(const void* cur_gb2, const void* cur_gb3, const void* prev_gb2, const void* prev_gb3, bool first_frame, int ping_pong = -1)
    {
        const bool had = history && valid;
        const bool handed_back = prev_gb2 == gb2 && prev_gb3 == gb3 && prev_gb2 != cur_gb2 && prev_gb3 != cur_gb3;
        Step s;
        s.read = (had && !first_frame && (ping_pong < 0 || ping_pong != pp) && handed_back) ? parity : -1;
        parity ^= 1;
        s.write = parity;
        s.require_failed = require && had && s.read < 0;
        valid = true; pp = ping_pong; gb2 = cur_gb2; gb3 = cur_gb3;
        return s;
    }
    static std::string require_message(const char* stage) { return std::string(stage) + ": HR_DEBUG_REQUIRE_GEO is set and the record path was not taken"; }
};

// ------------------------------------------------------------------------------------------------ residency cap
// kf_shadows_atrous01 (denoise_fast_shadows.hip): how many bytes of unused dynamic LDS a launch asks for so that a CU holds at most R of its
// workgroups.  The live workgroups of a launch (30 % at the 1080p bench frame; the others leave after a scalar vote) have all started
// within its first 5 us, 2 to 8 of them to a CU, and the launch lasts as long as the CU that was dealt the most (measured: tools/
// atrous_balance.py, docs/EXPERIMENTS.md "live workgroups per CU"): the pad bounds how many a CU runs at a time.  static + pad = the largest size, a multiple of the allocation granule, of which R fit into a CU's LDS (if the
// granule is too coarse for any multiple to give exactly R: the largest size as such).  0 when the kernel's own LDS already allows R or
// fewer (a pad can only lower the residency), or R <= 0.  R >= 3: static + pad <= lds_per_cu / 3, within the 64 KiB a workgroup may ask for.
inline int atrous_resident_pad(int lds_per_cu, int static_bytes, int R, int granule)
{
    if (R < 3 || lds_per_cu <= 0 || static_bytes < 0 || granule <= 0) return 0;
    const int own = (static_bytes + granule - 1) / granule * granule;      // what the kernel's own LDS occupies
    if (own > 0 && lds_per_cu / own <= R) return 0;
    const int most = lds_per_cu / R;                                       // R of these fit, R + 1 of anything at most (R / (R + 1)) of it do
    int total = most / granule * granule;
    if (total <= 0 || lds_per_cu / total != R) total = most;
    return total > static_bytes ? total - static_bytes : 0;
}

} // namespace hr

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------------ PassCore
#include "hr_internal.h"
#include "pass_args.h"
#include "tile_order.h"
#include <cstdlib>
#include <vector>

namespace hr {

// What hr_shadows, hr_ao and hr_reflections derive from.  The extern "C" entry points stay in the pass files and forward here where the body
// is common; anything that differs between the passes (their images, kernels and argument blocks) stays there.
struct PassCore : PassRows
{
    hr_ctx*       ctx = nullptr;
    StageProfiler prof;
    hipStream_t   last_stream = nullptr;
    TileOrder     tile_order;          // heaviest-first launch order of the trace kernel (tile_order.h)
    bool          first_frame = true, last_denoise = true, want_stats = false;
    bool          fuse = true;         // tolerance mode: the pass's fused denoise launch (developer A/B switch HR_FUSE=0, read once at create)
    GeoRecords    records;
    DevBuf        upsample, tile_class, counters, ray_slots;

    // row bands only: the word a temporal kernel sets when a history tap falls on a row this GPU does not hold
    uint32_t* apron_flag() const { return banded() ? (uint32_t*)((char*)counters.p + 48) : nullptr; }
};

// hr_*_create up to the allocations: argument check, device, the switches every pass reads from the environment (once: the render path never
// calls getenv), the rows.  On success *made is a new Pass, which the caller deletes if a later step fails.
template <class Pass>
hr_status pass_new(Pass** made, hr_ctx* ctx, int32_t full_width, int32_t full_height, hr_scale scale, const hr_band* band, Pass** out, BandRule rule, const char* tag)
{
    HR_CHECK_ARG(ctx && out && full_width > 0 && full_height > 0 && (int)scale >= 0 && (int)scale <= 2);
    HR_HIP(hipSetDevice(ctx->device));
    Pass* p = new Pass();
    p->ctx = ctx;
    if (const char* e = getenv("HR_FUSE")) p->fuse = atoi(e) != 0;
    if (const char* e = getenv("HR_GEO_HISTORY")) p->records.history = atoi(e) != 0;
    if (const char* e = getenv("HR_DEBUG_REQUIRE_GEO")) p->records.require = atoi(e) != 0;
    if (const char* e = getenv("HR_TILE_ORDER")) p->tile_order.enabled = atoi(e) != 0;
    p->tile_order.tag = tag;
    if (const char* why = p->init(full_width, full_height, (int)scale, band, rule))
    {
        set_last_error(why);
        delete p;
        return HR_ERR_INVALID_ARG;
    }
    *made = p;
    return HR_OK;
}
// allocate-or-give-up inside hr_*_create (`p` the new pass, `s` an hr_status)
#define HR_PASS_ALLOC(buf, n) if ((s = p->buf.alloc(n)) != HR_OK) { delete p; return s; }

template <class Pass>
hr_status pass_destroy(Pass* p)
{
    if (!p) return HR_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipDeviceSynchronize();
    delete p;
    return HR_OK;
}

inline hr_status pass_reset_history(PassCore* p)
{
    HR_CHECK_ARG(p);
    p->first_frame = true;
    p->records.invalidate();
    p->tile_order.invalidate();   // costs of a frame that may never have run are not sorted (the launch list itself is always a permutation)
    return HR_OK;
}

// Row bands: did any history tap of the frames rendered since the last call fall on an image row this GPU does not hold (per-frame
// motion beyond hr_band.history_halo)?  Such taps were treated as disoccluded — the image stays valid but is no longer identical to
// the single-GPU one; the integrator widens history_halo (or re-creates the band) when this fires.  Synchronises the stream.
inline hr_status pass_history_apron_exceeded(PassCore* p, int32_t* exceeded)
{
    HR_CHECK_ARG(p && exceeded);
    uint32_t v = 0;
    HR_HIP(hipStreamSynchronize(p->last_stream));
    HR_HIP(hipMemcpy(&v, (char*)p->counters.p + 48, 4, hipMemcpyDeviceToHost));
    if (v) HR_HIP(hipMemset((char*)p->counters.p + 48, 0, 4));
    *exceeded = v ? 1 : 0;
    return HR_OK;
}

inline hr_status pass_set_profiling(PassCore* p, int32_t enable) { HR_CHECK_ARG(p); p->prof.enabled = enable != 0; return HR_OK; }
inline hr_status pass_get_stage_times(PassCore* p, hr_stage_times* out) { HR_CHECK_ARG(p && out); p->prof.collect(out); return HR_OK; }
inline hr_status pass_launch_order(PassCore* p, uint32_t* out, int32_t* n_tiles) { HR_CHECK_ARG(p); return p->tile_order.read(out, n_tiles, p->last_stream); }

// rays fired by the last trace: the sum of the per-tile slots (Slot: uint16_t in the shadow pass, uint32_t in the other two)
template <class Slot>
hr_status pass_ray_count(PassCore* p, uint64_t* rays)
{
    HR_CHECK_ARG(p && rays);
    HR_HIP(hipStreamSynchronize(p->last_stream));
    std::vector<Slot> slots((size_t)p->tiles_x * p->tiles_y);
    HR_HIP(hipMemcpy(slots.data(), p->ray_slots.p, slots.size() * sizeof(Slot), hipMemcpyDeviceToHost));
    uint64_t total = 0;
    for (Slot v : slots) total += v;
    *rays = total;
    return HR_OK;
}

inline hr_status check_inputs(const PassCore* p, const hr_frame_inputs* in, bool need_prev)
{
    HR_CHECK_ARG(in->cur.depth && in->cur.gb2 && in->cur.gb3);
    HR_CHECK_ARG(in->cur.width == p->w && in->cur.height == p->h);
    if (need_prev) HR_CHECK_ARG(in->prev.depth && in->prev.gb2 && in->prev.gb3 && in->prev.width == p->w && in->prev.height == p->h);
    return HR_OK;
}

inline hr_status geo_require_error(const char* stage)
{
    set_last_error(GeoRecords::require_message(stage));
    return HR_ERR_INVALID_ARG;
}

// hr_*_upsample of a scaled pass: `src` (fp16, in_channels per texel) to the full-resolution `upsample` image
inline hr_status pass_upsample(PassCore* p, const hr_frame_inputs* in, bool exact, const void* src, int in_channels, int channels, float sky_value, float power, uint64_t algorithmic_bytes, void* stream_)
{
    if (p->scale == 0) return HR_OK; // ray_traced_shadows.cpp:113
    HR_CHECK_ARG(in->cur_full.gb2 && in->cur_full.gb3 && in->cur_full.width == p->full_w && in->cur_full.height == p->full_h);
    hipStream_t st = (hipStream_t)stream_;
    p->last_stream = st;
    UpsampleArgs a;
    a.W = p->full_w; a.H = p->full_h; a.w = p->w; a.h = p->h;
    a.G2 = (const uint2*)in->cur_full.gb2; a.G3 = (const uint2*)in->cur_full.gb3;
    a.g2 = (const uint2*)in->cur.gb2; a.g3 = (const uint2*)in->cur.gb3;
    a.in = src; a.in_channels = in_channels; a.channels = channels;
    a.out = p->upsample.p; a.sky_value = sky_value; a.power = power;
    int ev = p->prof.begin("upsample", st, algorithmic_bytes);
    if (exact) launch_upsample(a, st);
    else launch_upsample_fast(a, st);
    p->prof.end(ev, st);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

} // namespace hr
#endif // __HIPCC__
