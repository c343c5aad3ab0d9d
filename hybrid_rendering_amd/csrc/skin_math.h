// The arithmetic of one skinned corner (include/hr_skin.h "Contract"), written ONCE for the kernel (skinning.hip k_skin_pose) and for the host
// restatement (hr_skin_pose_host).  Both sides compile with -ffp-contract=off; every operation below is one IEEE fp32 + * / sqrt, a comparison
// or a select, sums are taken in the order written, so host and device produce the same bits.  Plain C++ when no HIP compiler is at work.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HR_HD __host__ __device__ inline
#else
#define HR_HD inline
#endif

namespace hr {
namespace skin {

// IEEE quotient and square root: device_math.h's helpers on the device (__fdiv_rn, hr_sqrt = __builtin_sqrtf), the host's own / and sqrt
HR_HD float div_rn(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
HR_HD float sqrt_rn(float x) { return __builtin_sqrtf(x); }
HR_HD bool  finite_f(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return (u & 0x7f800000u) != 0x7f800000u; }

// The caller's palette as it lies in memory: [n_joints][16] column-major, the last row is not read.  row(j, r, out): J[j][r][0..3].
struct PaletteColumnMajor
{
    const float* m;
    HR_HD void row(int j, int r, float* out) const
    {
        const float* p = m + (long long)j * 16 + r;
        out[0] = p[0]; out[1] = p[4]; out[2] = p[8]; out[3] = p[12];
    }
};

// "Morph": v = v + mw * d, the product rounded, then the sum
HR_HD void morph3(float* v, float mw, const float* d)
{
    const float a = mw * d[0], b = mw * d[1], c = mw * d[2];
    v[0] = v[0] + a; v[1] = v[1] + b; v[2] = v[2] + c;
}

// "Blend": M[r][c] (row-major 3x4) over the slots whose weight is not zero, in slot order.  A slot with w == 0 (+0 or -0) is not read at all:
// its joint index may be anything and its matrix need not be finite.  No live slot (hr_skin_check_desc refuses it): M = 0.
template <class Palette>
HR_HD void blend(const uint16_t* joint /*[4]*/, const float* w /*[4]*/, const Palette& pal, float* M /*[12]*/)
{
    for (int q = 0; q < 12; q++) M[q] = 0.0f;
    bool first = true;
    for (int k = 0; k < 4; k++)
    {
        const float wk = w[k];
        if (wk != 0.0f)
        {
            for (int r = 0; r < 3; r++)
            {
                float J[4];
                pal.row((int)joint[k], r, J);
                for (int c = 0; c < 4; c++)
                {
                    const float T = wk * J[c];
                    M[r * 4 + c] = first ? T : M[r * 4 + c] + T;
                }
            }
            first = false;
        }
    }
}

// "Position": out[r] = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3]
HR_HD void position(const float* M, const float* p, float* out)
{
    for (int r = 0; r < 3; r++) out[r] = ((M[r * 4 + 0] * p[0] + M[r * 4 + 1] * p[1]) + M[r * 4 + 2] * p[2]) + M[r * 4 + 3];
}

// "Normal": mat3(M) n, divided by its length when the squared length is positive and finite, stored as it stands otherwise
HR_HD void normal(const float* M, const float* n, float* out)
{
    float v[3];
    for (int r = 0; r < 3; r++) v[r] = (M[r * 4 + 0] * n[0] + M[r * 4 + 1] * n[1]) + M[r * 4 + 2] * n[2];
    const float l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (l2 > 0.0f && finite_f(l2))
    {
        const float l = sqrt_rn(l2);
        v[0] = div_rn(v[0], l); v[1] = div_rn(v[1], l); v[2] = div_rn(v[2], l);
    }
    out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
}

} // namespace skin
} // namespace hr
