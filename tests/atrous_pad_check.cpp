// csrc/pass_core.h atrous_resident_pad without a GPU: the bytes of unused dynamic LDS that bound how many workgroups of kf_shadows_atrous01 a
// CU holds.  A program of its own (tests/test_atrous_pad_host.py builds and runs it).  What is asserted follows from the definition, not from
// what the function returns:
//   * with byte granularity, whenever R workgroups of the kernel's own LDS fit at all (R * static <= LDS), exactly R of (static + pad) fit:
//     floor(LDS / (static + pad)) == R, and static + pad stays within the 64 KiB a workgroup may ask for;
//   * with the hardware's granule (1280 B on gfx950; 512 B on its predecessors), the same holds for what the hardware allocates,
//     static + pad rounded up to the granule, wherever a multiple of the granule with exactly R fitting exists;
//   * a pad never raises the residency: when the kernel's own LDS already allows R or fewer, the pad is 0.
#include "pass_core.h"
#include <cstdio>

using namespace hr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { if (g_failed++ < 20) printf("FAILED %s:%d: %s (lds %d static %d R %d granule %d pad %d)\n", __FILE__, __LINE__, #cond, lds, st, R, g, pad); } } while (0)

int main()
{
    const int limit = 65536;
    const int granules[3] = { 1, 512, 1280 };
    for (int lds = 64 * 1024; lds <= 160 * 1024; lds += 16 * 1024)
        for (int st = 0; st <= 40000; st += 400)
            for (int R = 3; R <= 8; R++)
                for (int gi = 0; gi < 3; gi++)
                {
                    const int g = granules[gi];
                    const int pad = atrous_resident_pad(lds, st, R, g);
                    const int own = (st + g - 1) / g * g;
                    CHECK(pad >= 0);
                    CHECK(st + pad <= limit);
                    if (own > 0 && lds / own <= R) { CHECK(pad == 0); continue; }   // the kernel alone allows R or fewer
                    const int total = st + pad, hw = (total + g - 1) / g * g;        // asked for / allocated
                    CHECK(total > 0 && lds / total == R);
                    const int best = lds / R / g * g;                                // the largest multiple of the granule of which R fit
                    if (best > 0 && lds / best == R) CHECK(lds / hw == R);
                }
    {
        // the kernel as built (19 600 B) on a CU of 160 KiB: 20 480 B allocated, 8 fit -> R = 8 needs no pad; R = 5: 32 000 B in all
        int lds = 160 * 1024, st = 19600, R = 8, g = 1280, pad = atrous_resident_pad(lds, st, R, g);
        CHECK(pad == 0);
        R = 5; pad = atrous_resident_pad(lds, st, R, g);
        CHECK(pad == 32000 - 19600);
        R = 2; pad = atrous_resident_pad(lds, st, R, g);   // below 3: more than 64 KiB per workgroup, out
        CHECK(pad == 0);
        R = 0; pad = atrous_resident_pad(lds, st, R, g);
        CHECK(pad == 0);
    }
    printf("pad: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
