// Tolerance-mode resolve kernels: the DDGI probe-grid sample and the upsample, and the self test of the tolerance-mode arithmetic
// (denoise_fast_common.h has what the units share).
#include "denoise_fast_common.h"
#include "ddgi_sample_fast.h"   // sets contract(fast) for its own bodies and ends with contract(off) ...
#include "selftest.h"

#pragma clang fp contract(fast)   // ... so this unit's kernels state it again: they are compiled as the other units' are

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// gi_sample_probe_grid.comp:75-99, tolerance mode; the 8-probe gather is ddgi_sample_fast.h (shared with the reflections' hit shading)
__global__ __launch_bounds__(256) void kf_ddgi_sample(DDGISampleArgs a)
{
    const uint2 BLK = block_xy<0>();
    const int x = BLK.x * 32 + (threadIdx.x & 31), y = a.y0 + BLK.y * 8 + (threadIdx.x >> 5);
    if (x >= a.w || y >= a.y1) return;
    const uint32_t o  = (uint32_t)(y * a.w + x);
    uint2* outp = reinterpret_cast<uint2*>(reinterpret_cast<char*>(a.out) + o * 8u);
    const float dp = fm::ld<float>(a.depth, o * 4u);
    if (dp == 1.0f) { *outp = make_uint2(0u, 0u); return; }
    const DDGIU& d = a.d;
    // (x + 0.5) / w correctly rounded (round 5, as in Reproj::issue): the clip -> world products cancel 3-4 digits, one ulp of tu moved P by up
    // to ~1e-3 (20 ulp of its coordinates) — more than the whole guard of the gather's knife-edge tests
    const float tu = fm::div_by_inrange((float)x + 0.5f, div_prepare((float)a.w)), tv = fm::div_by_inrange((float)y + 0.5f, div_prepare((float)a.h));
    const f3 P  = fm::unproject_at(fm::unproject_base(a.vpi, tu, tv), a.vpi, dp);
    const f3 N  = fm::oct_unit(fm::ld<uint32_t>(a.gb2, o * 8u));
    f3       Wo = mk3(a.cam[0] - P.x, a.cam[1] - P.y, a.cam[2] - P.z);
    const float iwo = fm::rsq(fm::dot(Wo, Wo));
    Wo = mk3(Wo.x * iwo, Wo.y * iwo, Wo.z * iwo);
    // the redo of a pixel with a probe on the Chebyshev knife edge needs k_ddgi_sample's own operands of this pixel (exact_predicates.h)
    auto exact_inputs = [&](f3& eP, f3& eN, f3& eWo) { exact::pixel_inputs(a.vpi, a.cam, x, y, a.w, a.h, dp, fm::ld<uint32_t>(a.gb2, o * 8u), eP, eN, eWo); };
#ifdef HR_DEBUG_DDGI_PIXEL   // developer build: -DHR_DEBUG_DDGI_PIXEL -DHR_DBG_X=.. -DHR_DBG_Y=.. -DHR_DBG_W=.. prints the gather's terms of one pixel
    const bool dbg = x == HR_DBG_X && y == HR_DBG_Y && a.w == HR_DBG_W;
#else
    const bool dbg = false;
#endif
    const f3 net = ddgi_fast::sample_irradiance_net<true>(d, P, N, Wo, a.irr, a.dep, exact_inputs, dbg);
    const float k = d.energy_preservation * (0.5f * HR_M_PI) * a.gi_intensity;
    *outp = make_uint2(fm::pack2(net.x * net.x * k, net.y * net.y * k), fm::pack2(net.z * net.z * k, 1.0f));
}

// ------------------------------------------------------------------------------------------------------------------------
// shadows_upsample.comp / ao_upsample.comp / reflections_upsample.comp, tolerance mode
template <int CH>
__global__ __launch_bounds__(256) void kf_upsample(UpsampleArgs a)
{
    const uint2 BLK = block_xy<0>();
    const int x = BLK.x * 32 + (threadIdx.x & 31), y = BLK.y * 8 + (threadIdx.x >> 5);
    if (x >= a.W || y >= a.H) return;
    const uint32_t o  = (uint32_t)(y * a.W + x);
    uint16_t*      op = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.out) + o * (2u * CH));
    const float hi_depth = fm::hi(fm::ld<uint32_t>(a.G3, o * 8u + 4u));
    if (hi_depth == -1.0f)
    {
        const uint16_t sv = fm::half_bits(a.sky_value);
#pragma unroll
        for (int c = 0; c < CH; c++) op[c] = sv;
        return;
    }
    const f3    hn = fm::oct_unit(fm::ld<uint32_t>(a.G2, o * 8u));
    // correctly rounded quotients (the texel addressing below is a discrete decision); the divisors are launch constants
    const float tu = fm::div_by_inrange((float)x + 0.5f, div_prepare((float)a.W)), tv = fm::div_by_inrange((float)y + 0.5f, div_prepare((float)a.H));
    const float tsx = fm::div_by_inrange(1.0f, div_prepare((float)a.w)), tsy = fm::div_by_inrange(1.0f, div_prepare((float)a.h));
    float up[CH], total_w = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; c++) up[c] = 0.0f;
    uint32_t t3[4], t2[4];
    uint16_t tin[4][CH];
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        const float kx = (i == 1) ? 1.0f : (i == 2 ? -1.0f : 0.0f), ky = (i == 0) ? 1.0f : (i == 3 ? -1.0f : 0.0f);
        int sx = fm::tap_texel(tu, kx, tsx, (float)a.w), sy = fm::tap_texel(tv, ky, tsy, (float)a.h);   // fast_math.h: the reference's rounding
        sx = clampi(sx, 0, a.w - 1); sy = clampi(sy, 0, a.h - 1);
        const uint32_t so = (uint32_t)(sy * a.w + sx);
        t3[i] = fm::ld<uint32_t>(a.g3, so * 8u + 4u); t2[i] = fm::ld<uint32_t>(a.g2, so * 8u);
        const uint16_t* ip = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(a.in) + so * (uint32_t)(2 * a.in_channels));
#pragma unroll
        for (int c = 0; c < CH; c++) tin[i][c] = ip[c];
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        const float cd = fm::hi(t3[i]);
        // compute_edge_stopping_weight, NORMAL weight only: wL = 1 (edge_stopping.glsl:53-59)
        const float wZ = fm::exp2f_(-__builtin_fabsf(hi_depth - cd) * 1.44269504088896341f);
        const float wN = fm::pow32(fm::sat(fm::dot(hn, fm::oct_unit(t2[i]))));
        const float wt = (cd == -1.0f) ? 0.0f : fm::exp2f_((1.0f + wZ) * -1.44269504088896341f) * wN;
#pragma unroll
        for (int c = 0; c < CH; c++) up[c] += (float)__builtin_bit_cast(_Float16, tin[i][c]) * wt;
        total_w += wt;
    }
    const float iw = fm::rcp(fm::fmax_(total_w, 0.00000001f));
#pragma unroll
    for (int c = 0; c < CH; c++)
    {
        float r = up[c] * iw;
        if (a.power != 0.0f) r = fm::powf_(r, a.power);
        op[c] = fm::half_bits(r);
    }
}

} // namespace

namespace hr {

void launch_ddgi_sample_fast(const DDGISampleArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(kf_ddgi_sample, dim3(grid_cols(cdiv(a.w, 32), 3), cdiv(a.y1 - a.y0, 8)), dim3(256), 0, st, a);
}

void launch_upsample_fast(const UpsampleArgs& a, hipStream_t st)
{
    const dim3 grid(grid_cols(cdiv(a.W, 32), 2), cdiv(a.H, 8));
    if (a.channels == 4) hipLaunchKernelGGL(kf_upsample<4>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(kf_upsample<1>, grid, dim3(256), 0, st, a);
}

} // namespace hr

// ---- self test of this translation unit's arithmetic (hr_selftest_fast_math, include/hr_api_post.h) --------------------------------
// Compiled here, under the contract(fast) pragma above, so that the parity helpers (fm::*_rn, exact::*) are checked where the tolerance
// kernels use them: their claim is that contraction stays off inside them whatever the surrounding code allows.
namespace hr {

HR_DEV void selftest_fast_eval(int which, const float v[8], const SelftestParams& P, float r[SELFTEST_MAX_OUT])
{
    const float x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int k = 0; k < SELFTEST_MAX_OUT; k++) r[k] = 0.0f;
    const int w = (int)P.w, h = (int)P.h;
    switch (which)
    {
        case 0: r[0] = fm::rcp(x); r[1] = fm::rsq(x); r[2] = fm::sqrt1(x); r[3] = fm::rcp_nr(x); break;
        case 1: r[0] = fm::expf_(x); r[1] = fm::log2f_(x); r[2] = fm::exp2f_(x); break;
        case 2: r[0] = fm::powf_(x, y); break;
        case 3: { const uint32_t p = fm::pack2(x, y); r[0] = (float)(p & 0xffffu); r[1] = (float)(p >> 16); break; }
        case 4:
        {
            const uint32_t p = (uint32_t)f2h(x) | ((uint32_t)f2h(y) << 16);
            const f3 a = fm::oct_raw(p), b = fm::oct_unit(p);
            r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = b.x; r[4] = b.y; r[5] = b.z;
            break;
        }
        case 5: r[0] = fm::mix_rn(x, y, z); r[1] = fm::var_rn(x, y); r[2] = fm::mad_rn(x, y, z); r[3] = fm::mul_rn(x, y); r[4] = fm::cheb_variance_rn(x, y); break;
        case 6: r[0] = fm::bilerp_rn(v[0], v[1], v[2], v[3], v[4], v[5]); break;
        case 7:
        {
            const DivBy Dw = div_prepare(v[5]), Dh = div_prepare(v[6]);
            fm::atlas_coord_rn(v[0], v[1], (int)v[2], (int)v[3], (int)v[4], v[5], v[6], Dw, Dh, r[0], r[1]);
            break;
        }
        case 8: r[0] = fm::div_rn(x, y); r[1] = (float)fm::tap_texel(x, y, z, v[3]); break;
        case 9:
        {
            const int px = (int)x, py = (int)y;
            r[0] = exact::tap_valid(P.m, px, py, w, h, z, __float_as_uint(v[3]), __float_as_uint(v[4]), P.cur_id, px, py, __float_as_uint(v[5]),
                                    __float_as_uint(v[6]), v[7]) ? 1.0f : 0.0f;
            break;
        }
        case 10: exact::virtual_point(P.m, P.m2, mk3(P.cam[0], P.cam[1], P.cam[2]), (int)x, (int)y, w, h, z, v[3], r[0], r[1]); break;
        case 11:
        {
            f3 Pw, N, Wo;
            exact::pixel_inputs(P.m, P.cam, (int)x, (int)y, w, h, z, __float_as_uint(v[3]), Pw, N, Wo);
            r[0] = Pw.x; r[1] = Pw.y; r[2] = Pw.z; r[3] = N.x; r[4] = N.y; r[5] = N.z; r[6] = Wo.x; r[7] = Wo.y; r[8] = Wo.z;
            break;
        }
        default: break;
    }
}

__global__ void kf_selftest_fast_math(int which, int gen, long long first, long long n, const float* in, SelftestParams P, int nout, float* out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v[8], r[SELFTEST_MAX_OUT];
    selftest_inputs(gen, i, first, in, P, v);
    selftest_fast_eval(which, v, P, r);
    selftest_store(i, n, nout, r, out);
}

} // namespace hr

extern "C" hr_status hr_selftest_fast_math(int32_t which, int32_t gen, int64_t first, int64_t n, const float* in, const float* params, int32_t nout, float* out,
                                           void* stream)
{
    using namespace hr;
    HR_CHECK_ARG(n >= 0 && params && nout >= 1 && nout <= SELFTEST_MAX_OUT && gen >= SELFTEST_GEN_ARRAY && gen <= SELFTEST_GEN_DIV);
    HR_CHECK_ARG(n == 0 || (out && (gen != SELFTEST_GEN_ARRAY || in)));
    if (n == 0) return HR_OK;
    SelftestParams P;
    std::memcpy(&P, params, sizeof(P));
    hipLaunchKernelGGL(kf_selftest_fast_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)which, (int)gen, (long long)first,
                       (long long)n, in, P, (int)nout, out);
    HR_HIP(hipGetLastError());
    return HR_OK;
}
