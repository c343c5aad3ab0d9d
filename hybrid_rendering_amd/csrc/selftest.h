// Self-test sweeps of the device arithmetic (hr_selftest_math_sweep in api.hip, hr_selftest_fast_math in denoise_fast_resolve.hip).
//
// An element's inputs v[0..7] come either from an array ([n][8] floats, gen 0) or from its index j = first + i, so that sweeps over all
// 2^32 fp32 patterns never move inputs across the bus; the CPU mirror of the tests regenerates the same inputs on the host.  Outputs are planar:
// out[k * n + i] for k < nout.  Test infrastructure only: no pass calls this.
#pragma once
#include <cstring>
#include "device_math.h"

namespace hr {

// 80 floats, passed by value (a uniform kernel argument); the layout is restated by the CPU mirror of the tests
struct SelftestParams
{
    float    m[16];      // world_pos_from_depth / tap_valid / virtual_point / pixel_inputs: view_proj_inverse
    float    m2[16];     // virtual_point: prev_view_proj
    float    cam[3];     // camera position
    float    y, z;       // gen 1 / 2 / 3: the second and third operands
    float    w, h;       // image extent (tap_valid, virtual_point, pixel_inputs)
    float    cur_id;     // tap_valid: the pixel's mesh id
    uint32_t d_first;    // gen 3: bits of the first denominator
    int32_t  n_num;      // gen 3: numerators per denominator
    float    num[32];    // gen 3: the numerators; a NaN entry draws a random one in [1e-12, 3e5] of either sign from the index
    float    pad[6];
};
static_assert(sizeof(SelftestParams) == 80 * 4, "SelftestParams layout");

enum { SELFTEST_GEN_ARRAY = 0, SELFTEST_GEN_BITS = 1, SELFTEST_GEN_HALF2 = 2, SELFTEST_GEN_DIV = 3, SELFTEST_MAX_OUT = 9 };

HR_DEV float selftest_random_numerator(uint64_t j)
{
    uint64_t z = j * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 29)) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 32;
    const uint32_t lo = 0x2b8cbcccu, hi = 0x48927c00u;   // bits of 1e-12f and 3e5f
    const uint32_t b  = lo + (uint32_t)((z & 0xffffffffull) % (uint64_t)(hi - lo + 1u));
    return __uint_as_float(b | ((uint32_t)(z >> 63) << 31));
}

HR_DEV void selftest_inputs(int gen, long long i, long long first, const float* __restrict__ in, const SelftestParams& P, float v[8])
{
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = 0.0f;
    const uint64_t j = (uint64_t)(first + i);
    if (gen == SELFTEST_GEN_ARRAY)
    {
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = in[i * 8 + k];
        return;
    }
    v[1] = P.y;
    v[2] = P.z;
    if (gen == SELFTEST_GEN_BITS) v[0] = __uint_as_float((uint32_t)j);
    else if (gen == SELFTEST_GEN_HALF2)
    {
        v[0] = h2f((uint16_t)(j & 0xffffu));
        v[1] = h2f((uint16_t)((j >> 16) & 0xffffu));
    }
    else if (gen == SELFTEST_GEN_DIV)
    {
        const uint64_t nn = (uint64_t)(P.n_num > 0 ? P.n_num : 1);
        const float    t  = P.num[j % nn];
        v[0] = t != t ? selftest_random_numerator(j) : t;
        v[1] = __uint_as_float(P.d_first + (uint32_t)(j / nn));
    }
}

HR_DEV void selftest_store(long long i, long long n, int nout, const float r[SELFTEST_MAX_OUT], float* __restrict__ out)
{
#pragma unroll
    for (int k = 0; k < SELFTEST_MAX_OUT; k++)
        if (k < nout) out[k * n + i] = r[k];
}

} // namespace hr
