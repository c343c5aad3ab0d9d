// The environment's derived inputs on MI355X — HIP replacement for what the reference takes from its framework on the GPU:
// dw::CubemapSHProjection, dw::CubemapPrefiler (re-run whenever the sun moves, main.cpp:975-990) and dw::BRDFIntegrateLUT (once,
// common.cpp:307).  The framework's shaders are not part of the reference tree, so the arithmetic is specified in include/hr_env.h
//  and restated in float32 numpy by tests/env_reference.py; every kernel below follows that text operation by operation.
#include "env_internal.h"
#include <cmath>
#include <new>

using namespace hr;

namespace {

constexpr int kMaxSkySize = 2048, kMaxLut = 512, kMaxSamples = 4096;

// hr_env.h "GGX half vector", in the tangent frame of the normal
HR_DEV f3 ggx_half(float r, float4 row)
{
    const float a = r * r, a2 = a * a;
    const float cos2 = __fdiv_rn(1.0f - row.x, 1.0f + (a2 - 1.0f) * row.x);
    const float ct = hr_sqrt(cos2), st = hr_sqrt(1.0f - ct * ct);
    return mk3(st * row.y, st * row.z, ct);
}

// hr_env.h "Sums over samples": the xor butterfly over the wave's 64 lanes; every lane ends with the same sum
HR_DEV float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// the wave's index in the grid as a scalar: one wave owns one output texel (blocks of 256 threads = 4 waves)
HR_DEV long long wave_index() { return (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Ht of every (level >= 1, sample): it depends on the descriptor alone, so it is computed once at creation; ht = [levels - 1][n]
__global__ __launch_bounds__(256) void k_env_ht(const float4* __restrict__ table, int n, int levels, float4* __restrict__ ht)
{
    const int i = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y + 1;
    if (i >= n || l >= levels) return;
    const float r = __fdiv_rn((float)l, (float)(levels - 1));
    const f3 h = ggx_half(r, table[i]);
    ht[(size_t)(l - 1) * n + i] = make_float4(h.x, h.y, h.z, 0.0f);
}

__global__ __launch_bounds__(256) void k_env_lut(const float4* __restrict__ table, int n, int lut, uint32_t* __restrict__ out)
{
    const long long tex = wave_index();
    if (tex >= (long long)lut * lut) return;
    const int lane = threadIdx.x & 63, ix = (int)(tex % lut), iy = (int)(tex / lut);
    const float nv = __fdiv_rn((float)ix + 0.5f, (float)lut), r = __fdiv_rn((float)iy + 0.5f, (float)lut);
    const f3    V = mk3(hr_sqrt(1.0f - nv * nv), 0.0f, nv);
    const float k = __fdiv_rn(r * r, 2.0f);
    float A = 0.0f, B = 0.0f;
    for (int i = lane; i < n; i += 64)
    {
        const f3    H  = ggx_half(r, table[i]);
        const float vh = dot3(V, H);
        const f3    L  = sub3(scale3(H, 2.0f * vh), V);
        const float nl = L.z, nh = H.z;
        if (nl > 0.0f)
        {
            const float g1v = __fdiv_rn(nv, nv * (1.0f - k) + k), g1l = __fdiv_rn(nl, nl * (1.0f - k) + k);
            const float gv  = __fdiv_rn((g1v * g1l) * vh, nh * nv);
            const float t   = 1.0f - vh;
            const float fc  = ((t * t) * (t * t)) * t;
            A = A + (1.0f - fc) * gv;
            B = B + fc * gv;
        }
    }
    A = wave_sum(A);
    B = wave_sum(B);
    if (lane == 0) out[tex] = pack_h2(__fdiv_rn(A, (float)n), __fdiv_rn(B, (float)n));
}

// level 0 of the chain: the sky at the texel direction (one thread per texel)
__global__ __launch_bounds__(256) void k_env_level0(CubeMap sky, int ps, uint2* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= 6LL * ps * ps) return;
    const int x = (int)(t % ps), y = (int)((t / ps) % ps), face = (int)(t / ((long long)ps * ps));
    const f3 c = sky.fetch(normalize3(texel_dir(face, x, y, ps)));
    out[t] = make_uint2(pack_h2(c.x, c.y), pack_h2(c.z, 1.0f));
}

// levels >= 1 of the chain, all in one launch: wave -> (level, face, y, x) in the chain's own texel order
__global__ __launch_bounds__(256) void k_env_prefilter(CubeMap sky, int ps, int levels, int n, const float4* __restrict__ ht, uint2* __restrict__ chain)
{
    long long t   = wave_index();
    long long off = 6LL * ps * ps;
    int       l   = 1;
    for (; l < levels; l++)
    {
        const long long cnt = 6LL * (ps >> l) * (ps >> l);
        if (t < cnt) break;
        t -= cnt;
        off += cnt;
    }
    if (l >= levels) return;
    const int s = ps >> l, lane = threadIdx.x & 63;
    const int x = (int)(t % s), y = (int)((t / s) % s), face = (int)(t / ((long long)s * s));
    const f3 N  = normalize3(texel_dir(face, x, y, s));
    const f3 up = fabsf(N.z) < 0.999f ? mk3(0.0f, 0.0f, 1.0f) : mk3(1.0f, 0.0f, 0.0f);
    const f3 T  = normalize3(cross3(up, N));
    const f3 B  = cross3(N, T);
    const float4* __restrict__ h_l = ht + (size_t)(l - 1) * n;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f;
    for (int i = lane; i < n; i += 64)
    {
        const float4 h  = h_l[i];
        const f3     H  = add3(add3(scale3(T, h.x), scale3(B, h.y)), scale3(N, h.z));
        const f3     L  = sub3(scale3(H, 2.0f * dot3(N, H)), N);
        const float  nl = dot3(N, L);
        if (nl > 0.0f)
        {
            const f3 c = sky.fetch(L);
            ar = ar + c.x * nl;
            ag = ag + c.y * nl;
            ab = ab + c.z * nl;
            aw = aw + nl;
        }
    }
    ar = wave_sum(ar); ag = wave_sum(ag); ab = wave_sum(ab); aw = wave_sum(aw);
    if (lane == 0) chain[off + t] = make_uint2(pack_h2(__fdiv_rn(ar, aw), __fdiv_rn(ag, aw)), pack_h2(__fdiv_rn(ab, aw), 1.0f));
}

constexpr int kShSums = 28;   // 9 coefficients x rgb, then the weight

// SH9, first half: one wave per (face, row) of the sky; rows = [6 * S][28]
__global__ __launch_bounds__(256) void k_env_sh_rows(CubeMap sky, float* __restrict__ rows)
{
    const long long row = wave_index();
    const int S = sky.S;
    if (row >= 6LL * S) return;
    const int face = (int)(row / S), y = (int)(row % S), lane = threadIdx.x & 63;
    float acc[kShSums];
#pragma unroll
    for (int j = 0; j < kShSums; j++) acc[j] = 0.0f;
    for (int x = lane; x < S; x += 64)
    {
        const f3    d   = texel_dir(face, x, y, S);
        const float r2  = dot3(d, d);
        const float wt  = __fdiv_rn(4.0f, r2 * hr_sqrt(r2));
        const f3    nrm = normalize3(d);
        const f3    c   = sky.fetch(nrm);
        float b[9];
        b[0] = 0.282095f;
        b[1] = -0.488603f * nrm.y;
        b[2] = 0.488603f * nrm.z;
        b[3] = -0.488603f * nrm.x;
        b[4] = (1.092548f * nrm.x) * nrm.y;
        b[5] = (-1.092548f * nrm.y) * nrm.z;
        b[6] = 0.315392f * (((3.0f * nrm.z) * nrm.z) - 1.0f);
        b[7] = (-1.092548f * nrm.x) * nrm.z;
        b[8] = 0.546274f * (nrm.x * nrm.x - nrm.y * nrm.y);
#pragma unroll
        for (int k = 0; k < 9; k++)
        {
            const float bw = b[k] * wt;
            acc[k * 3 + 0] = acc[k * 3 + 0] + c.x * bw;
            acc[k * 3 + 1] = acc[k * 3 + 1] + c.y * bw;
            acc[k * 3 + 2] = acc[k * 3 + 2] + c.z * bw;
        }
        acc[27] = acc[27] + wt;
    }
#pragma unroll
    for (int j = 0; j < kShSums; j++) acc[j] = wave_sum(acc[j]);
    if (lane < kShSums)
    {
        float v = acc[0];
#pragma unroll
        for (int j = 1; j < kShSums; j++) v = lane == j ? acc[j] : v;
        rows[row * kShSums + lane] = v;
    }
}

// SH9, second half: the row results in (face, row) order — one wave, lane j adds sum j, so every sum sees the written order — then the scale
__global__ __launch_bounds__(64) void k_env_sh_final(const float* __restrict__ rows, int n_rows, float* __restrict__ sh9)
{
    const int j = threadIdx.x;
    float v = 0.0f;
    if (j < kShSums)
    {
        // eight loads in flight, then their eight additions in row order: the chain of additions is the written one, the loads no longer wait on it
        int r = 0;
        for (; r + 8 <= n_rows; r += 8)
        {
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; i++) t[i] = rows[(size_t)(r + i) * kShSums + j];
#pragma unroll
            for (int i = 0; i < 8; i++) v = v + t[i];
        }
        for (; r < n_rows; r++) v = v + rows[(size_t)r * kShSums + j];
    }
    const float wsum  = __shfl(v, kShSums - 1, 64);
    const float scale = __fdiv_rn(4.0f * HR_M_PI, wsum);
    if (j < 27) sh9[(j / 3) * 4 + (j % 3)] = v * scale;
    else if (j < 36) sh9[(j - 27) * 4 + 3] = 0.0f;
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
int  log2i(int v) { int l = 0; while ((1 << (l + 1)) <= v) l++; return l; }
bool samples_ok(int n) { return n >= 64 && n <= kMaxSamples && n % 64 == 0; }

uint32_t bitreverse32(uint32_t v)
{
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    return (v >> 16) | (v << 16);
}

// hr_env.h "Sample table"
void sample_table(int n, float* out)
{
    for (int i = 0; i < n; i++)
    {
        const float  xi1 = (float)i / (float)n;
        const float  xi2 = (float)bitreverse32((uint32_t)i) * 2.3283064365386963e-10f;   // 2^-32
        const double phi = 2.0 * 3.14159265358979323846 * (double)xi2;
        out[i * 4 + 0] = xi1;
        out[i * 4 + 1] = (float)std::cos(phi);
        out[i * 4 + 2] = (float)std::sin(phi);
        out[i * 4 + 3] = 0.0f;
    }
}

} // namespace

// what every update enqueues behind its write of the sky (hr_env_update's copy, env_sources.hip's two kernels)
hr_status hr::env_enqueue_derived(hr_env* e, hipStream_t st)
{
    const int S = e->d.sky_size, P = e->d.prefiltered_size, levels = e->d.prefiltered_levels, n = e->d.n_samples;
    const CubeMap sky { (const uint2*)e->sky.p, S };
    int ev = e->prof.begin("env_sh9", st, e->sky.bytes);
    hipLaunchKernelGGL(k_env_sh_rows, dim3(cdiv(6 * S, 4)), dim3(256), 0, st, sky, (float*)e->sh_rows.p);
    hipLaunchKernelGGL(k_env_sh_final, dim3(1), dim3(64), 0, st, (const float*)e->sh_rows.p, 6 * S, (float*)e->sh9.p);
    e->prof.end(ev, st);
    ev = e->prof.begin("env_prefilter", st, e->sky.bytes + e->chain.bytes);
    hipLaunchKernelGGL(k_env_level0, dim3((unsigned)(((size_t)6 * P * P + 255) / 256)), dim3(256), 0, st, sky, P, (uint2*)e->chain.p);
    const size_t waves = e->chain_texels - (size_t)6 * P * P;
    if (waves) hipLaunchKernelGGL(k_env_prefilter, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, sky, P, levels, n, (const float4*)e->ht.p, (uint2*)e->chain.p);
    e->prof.end(ev, st);
    HR_HIP(hipGetLastError());
    return HR_OK;
}

extern "C" {

void hr_env_default_desc(hr_env_desc* d)
{
    if (!d) return;
    d->sky_size = 128; d->prefiltered_size = 128; d->prefiltered_levels = 5; d->brdf_lut_size = 128; d->n_samples = 1024;
}

hr_status hr_env_sample_table(int32_t n, float* host_out)
{
    HR_CHECK_ARG(host_out && samples_ok(n));
    sample_table(n, host_out);
    return HR_OK;
}

hr_status hr_env_create(hr_ctx* ctx, const hr_env_desc* d, hr_env** out)
{
    HR_CHECK_ARG(d && out);   // the descriptor first: its checks need no device
    HR_CHECK_ARG(pow2(d->sky_size) && d->sky_size >= 4 && d->sky_size <= kMaxSkySize);
    HR_CHECK_ARG(pow2(d->prefiltered_size) && d->prefiltered_size <= d->sky_size);
    HR_CHECK_ARG(d->prefiltered_levels >= 1 && d->prefiltered_levels <= log2i(d->prefiltered_size) + 1);
    HR_CHECK_ARG(d->brdf_lut_size >= 1 && d->brdf_lut_size <= kMaxLut);
    HR_CHECK_ARG(samples_ok(d->n_samples));
    HR_CHECK_ARG(ctx);
    HR_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<hr_env> e(new (std::nothrow) hr_env());
    if (!e) return HR_ERR_OUT_OF_MEMORY;
    e->ctx = ctx; e->d = *d;
    const int S = d->sky_size, P = d->prefiltered_size, levels = d->prefiltered_levels, lut = d->brdf_lut_size, n = d->n_samples;
    for (int l = 0; l < levels; l++) e->chain_texels += (size_t)6 * (P >> l) * (P >> l);
    hr_status s;
    if ((s = e->sky.alloc((size_t)6 * S * S * 8)) != HR_OK) return s;
    if ((s = e->chain.alloc(e->chain_texels * 8)) != HR_OK) return s;
    if ((s = e->lut.alloc((size_t)lut * lut * 4)) != HR_OK) return s;
    if ((s = e->sh9.alloc(36 * sizeof(float))) != HR_OK) return s;
    if ((s = e->sh_rows.alloc((size_t)6 * S * kShSums * sizeof(float))) != HR_OK) return s;
    if ((s = e->table.alloc((size_t)n * 16)) != HR_OK) return s;
    if ((s = e->ht.alloc((size_t)(levels > 1 ? levels - 1 : 1) * n * 16)) != HR_OK) return s;
    std::vector<float> host((size_t)n * 4);
    sample_table(n, host.data());
    HR_HIP(hipMemcpy(e->table.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (levels > 1) hipLaunchKernelGGL(k_env_ht, dim3(cdiv(n, 256), levels - 1), dim3(256), 0, nullptr, (const float4*)e->table.p, n, levels, (float4*)e->ht.p);
    // the LUT is integrated here, once; its stage time is kept for the first hr_env_get_stage_times
    e->prof.enabled = true;
    const int ev = e->prof.begin("env_brdf_lut", nullptr, (uint64_t)lut * lut * 4);
    hipLaunchKernelGGL(k_env_lut, dim3(cdiv(lut * lut, 4)), dim3(256), 0, nullptr, (const float4*)e->table.p, n, lut, (uint32_t*)e->lut.p);
    e->prof.end(ev, nullptr);
    e->prof.enabled = false;
    HR_HIP(hipGetLastError());
    HR_HIP(hipStreamSynchronize(nullptr));
    *out = e.release();
    return HR_OK;
}

hr_status hr_env_destroy(hr_env* e)
{
    if (!e) return HR_OK;
    (void)hipSetDevice(e->ctx->device);
    (void)hipDeviceSynchronize();
    delete e;
    return HR_OK;
}

hr_status hr_env_set_profiling(hr_env* e, int32_t on) { HR_CHECK_ARG(e); e->prof.enabled = on != 0; return HR_OK; }
hr_status hr_env_get_stage_times(hr_env* e, hr_stage_times* out) { HR_CHECK_ARG(e && out); e->prof.collect(out); return HR_OK; }

hr_status hr_env_update(hr_env* e, const void* sky_device, void* stream)
{
    HR_SCOPED_SAMPLE("Environment Update");
    HR_CHECK_ARG(e && sky_device);
    HR_HIP(hipSetDevice(e->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    e->prof.begin_frame();
    HR_HIP(hipMemcpyAsync(e->sky.p, sky_device, e->sky.bytes, hipMemcpyDeviceToDevice, st));
    return env_enqueue_derived(e, st);
}

hr_status hr_env_get(const hr_env* e, hr_environment* out)
{
    HR_CHECK_ARG(e && out);
    out->sky = e->sky.p; out->sky_size = e->d.sky_size;
    out->prefiltered = e->chain.p; out->prefiltered_size = e->d.prefiltered_size; out->prefiltered_levels = e->d.prefiltered_levels;
    out->brdf_lut = e->lut.p; out->brdf_lut_size = e->d.brdf_lut_size;
    return HR_OK;
}

hr_status hr_env_sh9_device(const hr_env* e, const float** out)
{
    HR_CHECK_ARG(e && out);
    *out = (const float*)e->sh9.p;
    return HR_OK;
}

hr_status hr_env_read_sh9(hr_env* e, float out[9][4])
{
    HR_CHECK_ARG(e && out);
    HR_HIP(hipSetDevice(e->ctx->device));
    HR_HIP(hipDeviceSynchronize());
    HR_HIP(hipMemcpy(out, e->sh9.p, 36 * sizeof(float), hipMemcpyDeviceToHost));
    return HR_OK;
}

} // extern "C"
