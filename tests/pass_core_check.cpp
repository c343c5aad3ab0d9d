// The plain part of csrc/pass_core.h without a GPU: pass rows under the two band rules, and the geometry-record state machine driven through
// scripted frame sequences per pass flavour.  A program of its own (tests/test_pass_core_host.py builds it with the address and
// undefined-behaviour sanitizers).  Every expected value is a literal, worked out by hand from hr_shadows_create / hr_ao_create /
// hr_reflections_create and the three hr_*_temporal as they were before the passes shared this header.
#include "pass_core.h"
#include <cstdio>
#include <cstring>

using namespace hr;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static const char* kShadowsText = "band rows must be multiples of 8 inside the pass image; halo a multiple of 8";
static const char* kAoText      = "band rows must be multiples of 8";

static bool rows_are(const PassRows& r, int w, int h, int y0, int y1, int b0, int b1, int ry0, int ry1, int tx, int ty, int mw, int mh)
{
    return r.w == w && r.h == h && r.y0 == y0 && r.y1 == y1 && r.band_y0 == b0 && r.band_y1 == b1 && r.ry0 == ry0 && r.ry1 == ry1 &&
           r.tiles_x == tx && r.tiles_y == ty && r.mw == mw && r.mh == mh;
}
static bool refused(int W, int H, hr_band b, BandRule rule, const char* text)
{
    PassRows r;
    const char* why = r.init(W, H, 0, &b, rule);
    return why && !strcmp(why, text);
}

static void rows()
{
    const BandRule S = BandRule::Shadows, A = BandRule::AoReflections;
    PassRows r;
    // no band: the rules differ in band_y1 only (the whole image / 0)
    CHECK(!r.init(64, 40, 0, nullptr, S) && rows_are(r, 64, 40, 0, 40, 0, 40, 0, 40, 8, 5, 8, 10));
    CHECK(r.full_w == 64 && r.full_h == 40 && r.scale == 0 && r.tile_y0() == 0 && r.resident_tiles_y() == 5 && r.resident_tiles() == 40 && !r.banded());
    CHECK(!r.init(64, 40, 0, nullptr, A) && rows_are(r, 64, 40, 0, 40, 0, 0, 0, 40, 8, 5, 8, 10) && !r.banded());
    // an empty band (band_y1 <= band_y0) is no band
    hr_band none { 16, 16, 8, 8 };
    CHECK(!r.init(64, 40, 0, &none, S) && rows_are(r, 64, 40, 0, 40, 0, 40, 0, 40, 8, 5, 8, 10));
    CHECK(!r.init(64, 40, 0, &none, A) && rows_are(r, 64, 40, 0, 40, 0, 0, 0, 40, 8, 5, 8, 10));
    // band 8..24, halo 8, history halo 16: resident rows 0..32; the shadow pass may read history from 0..40
    hr_band b { 8, 24, 8, 16 };
    CHECK(!r.init(64, 40, 0, &b, S) && rows_are(r, 64, 40, 0, 32, 8, 24, 0, 40, 8, 5, 8, 10));
    CHECK(r.tile_y0() == 0 && r.resident_tiles_y() == 4 && r.resident_tiles() == 32 && r.banded());
    CHECK(!r.init(64, 40, 0, &b, A) && rows_are(r, 64, 40, 0, 32, 8, 24, 0, 32, 8, 5, 8, 10) && r.banded());
    // the last band of a 44-row image ends on the ragged row 44
    hr_band last { 16, 44, 8, 8 };
    CHECK(!r.init(64, 44, 0, &last, S) && rows_are(r, 64, 44, 8, 44, 16, 44, 8, 44, 8, 6, 8, 11));
    CHECK(r.tile_y0() == 1 && r.resident_tiles_y() == 5 && r.resident_tiles() == 40 && r.banded());
    CHECK(!r.init(64, 44, 0, &last, A) && rows_are(r, 64, 44, 8, 44, 16, 44, 8, 44, 8, 6, 8, 11));
    hr_band ragged { 16, 36, 0, 0 };   // ... but a ragged row inside the image is refused
    CHECK(refused(64, 44, ragged, S, kShadowsText) && refused(64, 44, ragged, A, kAoText));
    // scaled passes: the shift truncates (66 >> 1 = 33, 42 >> 1 = 21; 66 >> 2 = 16, 42 >> 2 = 10)
    CHECK(!r.init(66, 42, 1, nullptr, S) && rows_are(r, 33, 21, 0, 21, 0, 21, 0, 21, 5, 3, 5, 6) && r.full_w == 66 && r.full_h == 42 && r.scale == 1);
    CHECK(!r.init(66, 42, 2, nullptr, A) && rows_are(r, 16, 10, 0, 10, 0, 0, 0, 10, 2, 2, 2, 3) && r.scale == 2);
    // refusals.  band_y0 = 4: both
    hr_band odd0 { 4, 24, 0, 0 };
    CHECK(refused(64, 40, odd0, S, kShadowsText) && refused(64, 40, odd0, A, kAoText));
    // halo = 4: the shadow rule refuses the halo itself; the other rule sees resident rows 4..28
    hr_band halo4 { 8, 24, 4, 4 };
    CHECK(refused(64, 40, halo4, S, kShadowsText) && refused(64, 40, halo4, A, kAoText));
    // ... and accepts band 4..36, whose halo of 4 brings the resident rows to 0..40
    hr_band odd_sum { 4, 36, 4, 4 };
    CHECK(refused(64, 40, odd_sum, S, kShadowsText));
    CHECK(!r.init(64, 40, 0, &odd_sum, A) && rows_are(r, 64, 40, 0, 40, 4, 36, 0, 40, 8, 5, 8, 10) && !r.banded());
    // band_y1 > h, band_y0 < 0: the shadow rule refuses; the other rule clamps the resident rows and keeps the band as given
    hr_band below { 24, 48, 0, 0 };
    CHECK(refused(64, 40, below, S, kShadowsText));
    CHECK(!r.init(64, 40, 0, &below, A) && rows_are(r, 64, 40, 24, 40, 24, 48, 24, 40, 8, 5, 8, 10) && r.tile_y0() == 3 && r.resident_tiles_y() == 2);
    hr_band above { -8, 16, 0, 0 };
    CHECK(refused(64, 40, above, S, kShadowsText));
    CHECK(!r.init(64, 40, 0, &above, A) && rows_are(r, 64, 40, 0, 16, -8, 16, 0, 16, 8, 5, 8, 10) && r.resident_tiles_y() == 2);
    hr_band neg_halo { 8, 24, -8, 0 };
    CHECK(refused(64, 40, neg_halo, S, kShadowsText));
}

static bool step_is(const GeoRecords::Step& s, int read, int write, bool failed) { return s.read == read && s.write == write && s.require_failed == failed; }

static void records()
{
    char        mem[6];   // six distinct addresses standing for three G-buffers' GB2 / GB3
    const void *A2 = mem + 0, *A3 = mem + 1, *B2 = mem + 2, *B3 = mem + 3, *C2 = mem + 4, *C3 = mem + 5;
    for (int require = 0; require <= 1; require++)
    {
        // shadows with history reads on, reflections: no ping-pong index
        GeoRecords g;
        g.require = require != 0;
        CHECK(step_is(g.advance(A2, A3, A2, A3, false), -1, 1, false));          // first frame: nothing to read, nothing missed
        CHECK(g.valid && g.gb2 == A2 && g.gb3 == A3 && g.parity == 1);
        CHECK(step_is(g.advance(B2, B3, A2, A3, false), 1, 0, false));           // handed back: read what the last frame wrote
        CHECK(step_is(g.advance(A2, A3, B2, B3, false), 0, 1, false));
        CHECK(step_is(g.advance(B2, B3, C2, C3, false), -1, 0, require != 0));   // prev is not what was cur: the caller's images
        CHECK(step_is(g.advance(C2, C3, B2, B3, false), 0, 1, false));           // ... and the frame after it has records again
        CHECK(step_is(g.advance(C2, C3, C2, C3, false), -1, 0, require != 0));   // one G-buffer rewritten in place: prev aliases cur
        CHECK(step_is(g.advance(A2, C3, C2, C3, false), -1, 1, require != 0));   // ... or one of its two images does
        CHECK(step_is(g.advance(B2, B3, A2, B3, false), -1, 0, require != 0));   // only GB2 handed back
        g.invalidate();
        CHECK(step_is(g.advance(A2, A3, B2, B3, false), -1, 1, false));          // after a reset a handed-back prev is no miss
        CHECK(step_is(g.advance(B2, B3, A2, A3, true), -1, 0, require != 0));    // a first frame over standing records does not read them
        // AO: the record holds the colour history of ping_pong's other slot
        GeoRecords ao;
        ao.require = require != 0;
        CHECK(step_is(ao.advance(A2, A3, A2, A3, false, 1), -1, 1, false));
        CHECK(step_is(ao.advance(B2, B3, A2, A3, false, 0), 1, 0, false));
        CHECK(step_is(ao.advance(A2, A3, B2, B3, false, 0), -1, 1, require != 0));   // ping_pong did not alternate
        CHECK(ao.pp == 0);
        CHECK(step_is(ao.advance(B2, B3, A2, A3, false, 1), 1, 0, false));
        // shadows with HR_GEO_HISTORY=0: the a-trous stages still get a slot per frame, no frame reads one, nothing is required
        GeoRecords off;
        off.history = false; off.require = require != 0;
        CHECK(step_is(off.advance(A2, A3, A2, A3, false), -1, 1, false));
        CHECK(step_is(off.advance(B2, B3, A2, A3, false), -1, 0, false));
        CHECK(step_is(off.advance(A2, A3, B2, B3, false), -1, 1, false));
        CHECK(step_is(off.advance(B2, B3, C2, C3, false), -1, 0, false));
    }
    CHECK(GeoRecords::require_message("hr_ao_temporal") == "hr_ao_temporal: HR_DEBUG_REQUIRE_GEO is set and the record path was not taken");
}

int main()
{
    rows();
    printf("rows: %d checks\n", g_checks);
    const int before = g_checks;
    records();
    printf("records: %d checks\n", g_checks - before);
    return g_failed ? 1 : 0;
}
