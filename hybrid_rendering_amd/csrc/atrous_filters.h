// The edge-stopping filters of the tolerance-mode denoisers: the shadows' SVGF a-trous body, the AO blur's 1-D pass and staging step, and
// the tables, EdgeK set-up and colour helpers that the reflections' a-trous kernels share with them.
// Included by denoise_fast_common.h AFTER its `#pragma clang fp contract(fast)` and after exact_predicates.h (the pragma is part of what
// these bodies compute; the parity helpers fm::*_rn keep their own roundings).
//
// A filter body is written over a TEXEL SOURCE: an object that yields, for an offset from the centre in units of the tap distance,
//     unit(xx, yy)   the packed value of the texel at (xx, yy) TEXELS from the centre (the 3x3 variance prefilter; (0, 0) = the centre),
//     tap(xx, yy)    the packed value of the tap at (xx, yy) x tap distance,
//     nz(xx, yy)     that tap's unit normal and linear z ((0, 0) = the centre's),
//     ok(xx, yy)     false: the tap gets weight 0 whatever its values (a staged source stores a zero normal instead and says true).
// The shadow kernels differ in where a texel comes from — register arrays filled by one batch of loads (atrous_gather_pixel) or a staged
// LDS tile (StagedTaps: kf_shadows_atrous_lds, kf_shadows_atrous01) — and not in what is done with it.  Kernels that keep a loop of their
// own take its steps from here: the run-time-radius tail of kf_shadows_atrous, and kf_ao_blur and the reflections' a-trous kernels, which
// the compiler treats worse through a body (docs/EXPERIMENTS.md, "One filter body per pass").
// The order of the floating-point operations below is part of the result (tests/test_gpu_fast_filters.py pins the bits), and so, for
// speed, is the order of the memory reads: a body reads what the kernels read, where they read it.  Lambdas handed to
// prefilter_variance capture BY VALUE: by reference the closure keeps a kernel's locals in memory long enough to change its code.
#pragma once

namespace {

// ---- tables ------------------------------------------------------------------------------------------------------------------------
// 3x3 gaussian of the variance prefilter (compute_variance_center, shadows_denoise_atrous.comp:65-88)
HR_DEV constexpr float prefilter_weight(int xx, int yy) { return xx == 0 ? (yy == 0 ? 0.25f : 0.125f) : (yy == 0 ? 0.125f : 0.0625f); }
// a-trous kernel 1, 2/3, 1/6 along each axis, keyed by |xx|, |yy| (radius <= 2)
HR_DEV constexpr float tap_weight(int xx, int yy)
{
    const int   axx = xx < 0 ? -xx : xx, ayy = yy < 0 ? -yy : yy;
    const float kx = axx == 0 ? 1.0f : (axx == 1 ? 2.0f / 3.0f : 1.0f / 6.0f);
    const float ky = ayy == 0 ? 1.0f : (ayy == 1 ? 2.0f / 3.0f : 1.0f / 6.0f);
    return kx * ky;
}
// tap t of the 8 of a radius-1 filter -> its offset in tap distances (row-major 3x3 without the centre)
struct TapXY { int xx, yy; };
HR_DEV constexpr TapXY tap_xy(int t) { return TapXY { (t < 4 ? t : t + 1) % 3 - 1, (t < 4 ? t : t + 1) / 3 - 1 }; }

template <class F>
HR_DEV float prefilter_variance(F variance_at)
{
    float var = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++)
    {
        const int xx = k % 3 - 1, yy = k / 3 - 1;
        var += variance_at(xx, yy) * prefilter_weight(xx, yy);
    }
    return var;
}

// ---- edge-stopping weight ----------------------------------------------------------------------------------------------------------
struct EdgeK { float kz, phi_n, inv_phi_l; bool n32; };
struct NZ { f3 n; float z; };   // unit normal, linear z
HR_DEV NZ nz_of(float4 q) { return NZ { mk3(q.x, q.y, q.z), q.w }; }
HR_DEV NZ nz_of(uint32_t oct, uint32_t id_z) { const float z = fm::hi(id_z); return NZ { fm::oct_unit(oct), z }; }   // a geometry record {oct normal, mesh id | linear z}

// the mode-independent part; inv_phi_l follows the variance prefilter (edge_luma)
HR_DEV EdgeK edge_setup(float sigma_depth, float phi_normal, bool n32)
{
    EdgeK k;
    k.kz    = 1.44269504088896341f * fm::rcp(sigma_depth);
    k.phi_n = phi_normal;
    k.n32   = n32;
    return k;
}
HR_DEV float edge_luma(float phi, float var) { return fm::rcp(phi * fm::sqrt1(fm::fmax_(0.0f, 1e-10f + var))); }

HR_DEV float edge_weight_fast(const EdgeK& k, float cd, float sd, f3 cn, f3 sn, float cl, float sl)
{
    // edge_stopping.glsl:31-62 (NORMAL + LUMA): exp(-max(wL, 0) - max(wZ, 0)) * wN with wZ = exp(-|dz| / sigma) — sic, the depth
    // WEIGHT is used as an exponent term upstream; kept
    const float wZ = fm::exp2f_(-__builtin_fabsf(cd - sd) * k.kz);
    const float dn = fm::sat(fm::dot(cn, sn));
    const float wN = k.n32 ? fm::pow32(dn) : fm::powf_(dn, k.phi_n);
    const float wL = __builtin_fabsf(cl - sl) * k.inv_phi_l;
    return fm::exp2f_((wL + wZ) * -1.44269504088896341f) * wN;
}

// a staged LDS tile as a texel source: values in `img` (row stride IW, centre index vi), decoded geometry in `geo` (row stride GW, centre
// index ci), taps at distance D.  A texel that is not to count was staged with a zero normal: its weight is exactly 0.
struct StagedTaps
{
    const uint32_t* img;
    const float4*   geo;
    int             IW, vi, GW, ci, D;
    HR_DEV uint32_t unit(int xx, int yy) const { return img[vi + yy * IW + xx]; }
    HR_DEV uint32_t tap(int xx, int yy) const { return img[vi + yy * D * IW + xx * D]; }
    HR_DEV NZ   nz(int xx, int yy) const { return nz_of(geo[ci + yy * D * GW + xx * D]); }
    HR_DEV bool ok(int, int) const { return true; }
};

// ---- shadows: shadows_denoise_atrous.comp:94-174 ---------------------------------------------------------------------------------------
struct ShadowSums
{
    float w, v, var;
    HR_DEV void add(const EdgeK& ek, const NZ& c, float cv, const NZ& t, uint32_t tap, float kk, bool ok)
    {
        const float sv = fm::lo(tap);
        float wv = fm::mul_rn(edge_weight_fast(ek, c.z, t.z, c.n, t.n, cv, sv), kk);
        if (!ok) wv = 0.0f;
        w += wv;
        v += wv * sv;
        var += (wv * wv) * fm::hi(tap);
    }
    HR_DEV uint32_t finish(float power) const
    {
        const float iw = fm::rcp(w);
        float ov = v * iw;
        const float ovar = var * (iw * iw);
        if (power != 0.0f) ov = fm::powf_(fm::fmax_(ov, 0.0f), power);
        return fm::pack2(ov, ovar);
    }
};

// One radius-1 evaluation: variance prefilter, luminance scale, eight taps, normalise, power, pack.  `edge` yields the EdgeK without
// inv_phi_l; it is called AFTER the prefilter (a kernel that evaluates the filter once sets it up there, one that evaluates it in loops
// hands in the one it set up before them).  A sky centre (linear z < 0) passes through: BRANCH = true leaves before the taps, false
// computes them and selects (a source whose taps are loaded already has nothing to skip, and a select keeps the wave straight).
template <bool BRANCH, class Src, class Edge>
HR_DEV uint32_t shadows_filter(const Src& s, Edge edge, float phi_visibility, float power)
{
    const uint32_t c   = s.unit(0, 0);
    const NZ       cnz = s.nz(0, 0);
    const float    var = prefilter_variance([=](int xx, int yy) { return fm::hi(s.unit(xx, yy)); });
    if (BRANCH && cnz.z < 0.0f) return c;
    const float cv = fm::lo(c);
    EdgeK ek = edge();
    ek.inv_phi_l = edge_luma(phi_visibility, var);
    ShadowSums sum { 1.0f, cv, fm::hi(c) };
#pragma unroll
    for (int t = 0; t < 8; t++)
    {
        const TapXY    o  = tap_xy(t);
        const uint32_t tv = s.tap(o.xx, o.yy);
        const NZ       tn = s.nz(o.xx, o.yy);
        sum.add(ek, cnz, cv, tn, tv, tap_weight(o.xx, o.yy), s.ok(o.xx, o.yy));
    }
    const uint32_t r = sum.finish(power);
    return BRANCH ? r : (cnz.z < 0.0f ? c : r);
}

// "fetch, decode, zero if not resident" of one texel of a staged tile (resident: inside the image and rows ry0 .. ry1), in its steps:
// where (a texel that is not resident is fetched at the first resident texel), then — after the fetch, which ShadowsStageBatch issues for a
// whole batch — decode and select
HR_DEV bool shadows_stage_where(const AtrousArgs& a, int gx, int gy, int ry0, int ry1, uint32_t& so)
{
    const bool res = gx >= 0 && gx < a.w && gy >= ry0 && gy < ry1;
    // select the coordinates, then one 24-bit multiply-add (rows and widths are far below 2^24).  `res ? gy * a.w + gx : ry0 * a.w` compiles
    // to a branch around a 64-bit v_mad whose unused high addend is whatever register comes to hand — the destination of the load
    // issued just before, which makes every load of a batch wait for the one in front of it.
    const uint32_t sx = res ? (uint32_t)gx : 0u, sy = res ? (uint32_t)gy : (uint32_t)ry0;
    so = __umul24(sy, (uint32_t)a.w) + sx;
    return res;
}
HR_DEV void shadows_stage_decode(bool res, uint32_t v, uint2 nd, uint32_t& s_in, float4& s_nz)
{
    const f3 n = fm::oct_unit(nd.x);
    s_in = res ? v : 0u;
    s_nz = res ? make_float4(n.x, n.y, n.z, fm::hi(nd.y)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// A staged tile of N texels, row length TW, fetched by 256 threads in ONE batch: load() requests every texel of this thread — ROUNDS of
// them, texel i = thread + 256 * round — before anything waits; a round past the tile's end requests the first resident texel, so that no
// load sits behind a branch.  store() decodes and writes the LDS tile.  The kernel puts whatever else belongs to the batch, and then
// __builtin_amdgcn_sched_barrier(0), between the two: one global round trip for the whole tile.
template <int ROUNDS, int TW, int N>
struct ShadowsStageBatch
{
    static_assert(ROUNDS * 256 >= N && (ROUNDS - 1) * 256 < N, "ROUNDS = ceil(N / 256)");
    uint32_t v[ROUNDS];
    uint2    nd[ROUNDS];
    bool     res[ROUNDS];
    // (gx0, gy0): the image position of the tile's texel 0
    HR_DEV void load(const AtrousArgs& a, int gx0, int gy0, int ry0, int ry1)
    {
#pragma unroll
        for (int r = 0; r < ROUNDS; r++)
        {
            const int i = (int)threadIdx.x + r * 256, cy = i / TW, cx = i - cy * TW;
            uint32_t  so;   // past the tile's end (the last round only): row ry1, which is not resident
            res[r] = shadows_stage_where(a, gx0 + cx, (r * 256 + 255 < N || i < N) ? gy0 + cy : ry1, ry0, ry1, so);
            v[r]   = fm::ld<uint32_t>(a.in.p, so * 4u);
            nd[r]  = fm::ld<uint2>(a.nd, so * 8u);
        }
    }
    HR_DEV void store(uint32_t* s_in, float4* s_nz) const
    {
#pragma unroll
        for (int r = 0; r < ROUNDS; r++)
        {
            const int i = (int)threadIdx.x + r * 256;
            uint32_t  sv;
            float4    sn;
            shadows_stage_decode(res[r], v[r], nd[r], sv, sn);
            if (r * 256 + 255 < N || i < N) { s_in[i] = sv; s_nz[i] = sn; }
        }
    }
};

// ---- reflections: reflections_denoise_atrous.comp:94-181 -------------------------------------------------------------------------------
HR_DEV f3    refl_colour(uint2 q) { return mk3(fm::lo(q.x), fm::hi(q.x), fm::lo(q.y)); }
HR_DEV float refl_luma(f3 c) { return fm::fmax_(0.299f * c.x + 0.587f * c.y + 0.114f * c.z, 0.0001f); }

// ---- AO: ao_denoise_bilateral_blur.comp:75-139 -----------------------------------------------------------------------------------------
HR_DEV float gaussian_weight_fast(float offset, float deviation)
{
    const float d2 = deviation * deviation;
    return fm::rsq(2.0f * HR_M_PI * d2) * fm::expf_(-(offset * offset) * fm::rcp(2.0f * d2));
}
// bilateral weight of one tap: gaussian (read from *gauss where the kernels always read it) x edge-stopping (depth + normal; cz / tz linear
// eye depth, dn the normals' dot product)
HR_DEV float ao_tap_weight(const float* gauss, float cz, float tz, float dn)
{
    const float wZ = fm::exp2f_(-__builtin_fabsf(cz - tz) * 1.44269504088896341f);
    const float wN = fm::pow32(fm::sat(dn));
    return *gauss * (fm::exp2f_((1.0f + wZ) * -1.44269504088896341f) * wN);
}
HR_DEV float ao_normalise(float total_ao, float total_w) { return total_ao * fm::rcp(fm::fmax_(total_w, 0.0001f)); }

// One 1-D pass over a staged tile: geometry at s_nz[ci + i * stride], values at val[vi + i * vstride], i = -RADIUS .. RADIUS.
template <int RADIUS>
HR_DEV float ao_blur_1d(const float4* s_nz, int ci, int stride, const float* val, int vi, int vstride, const float* s_gauss)
{
    const float4 c = s_nz[ci];
    float total_ao = val[vi], total_w = 1.0f;
#pragma unroll
    for (int i = -RADIUS; i <= RADIUS; i++)
    {
        if (i == 0) continue;
        const float4 t = s_nz[ci + i * stride];
        const float  w = ao_tap_weight(&s_gauss[i + RADIUS], c.w, t.w, c.x * t.x + c.y * t.y + c.z * t.z);
        total_ao += w * val[vi + i * vstride];
        total_w += w;
    }
    return ao_normalise(total_ao, total_w);
}

// One texel of the blur's staged tile: fetch (resident: inside the image's columns and the band's rows; else a resident address whose values
// read as 0, the pinned rule), decode, store.  `note(ok, px, py, z)` runs between the loads and the decode, with the depth as fetched: the
// place where kf_ao_blur_xy classifies the texel (s_kind).
template <class Note>
HR_DEV void ao_stage_texel(const AOBlurArgs& a, int px, int py, float4& s_nz, float& s_ao, Note note)
{
    const bool ok = !(px < 0 || py < a.y0 || px >= a.w || py >= a.y1);
    const uint32_t off = ok ? (uint32_t)(py * a.w + px) : (uint32_t)(a.y0 * a.w);
    float    z  = fm::ld<float>(a.depth.p, off * 4u);
    uint32_t g2 = fm::ld<uint32_t>(a.gb2.p, off * 8u);
    uint16_t v  = fm::ld<uint16_t>(a.in.p, off * 2u);
    note(ok, px, py, z);
    if (!ok) { z = 0.0f; g2 = 0u; v = 0; }          // texel fetches outside the image read 0 (pinned rule), then decode as usual
    const f3 n = fm::oct_unit(g2);
    s_nz = make_float4(n.x, n.y, n.z, fm::rcp_nr(fm::mad_rn(a.zbp[2], z, a.zbp[3])));
    s_ao = (float)__builtin_bit_cast(_Float16, v);
}

} // namespace
