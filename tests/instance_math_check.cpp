// Stand-alone host check of hybrid_rendering_amd/csrc/instance_math.h (tests/test_instances_shared_device_host.py builds it with
// -fsanitize=address,undefined and runs it; nothing of it is loaded into Python).  Three things:
//   1. the header's bit-level helpers against <cmath>: next_down / next_up against std::nextafter, exponent_for against its definition;
//   2. record_terms and world_box over hostile matrices against a restatement with <cmath> calls (what instances_shared.hip fill_record and
//      instances.hip instance_boxes were before they called the header);
//   3. the refit of a 601-instance top level depth by depth, deepest first (the order of the device kernels), against the host's order
//      (slots from the last to the first): the same node bytes, boxes and areas; and every node against a <cmath> restatement of the node body
//      (exponents, quantisation, clamps) as refit_shared_top had it, extreme extents included.
// Prints one line per part and exits non-zero on the first difference.
#include "instance_math.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace hr;

static int fail(const char* what, int i)
{
    std::printf("FAIL %s at %d\n", what, i);
    return 1;
}

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static float    uni(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65535.0f; }

// ---- 2: the <cmath> restatements ---------------------------------------------------------------------------------------------------------------
static void ref_record(const float* m, const float* am, float* inv, float* iar, float* extent_out, uint32_t* flags)
{
    double A[3][3], C[3][3];
    for (int c = 0; c < 3; c++) for (int q = 0; q < 3; q++) A[q][c] = (double)m[c * 4 + q];
    C[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1]; C[0][1] = A[0][2] * A[2][1] - A[0][1] * A[2][2]; C[0][2] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
    C[1][0] = A[1][2] * A[2][0] - A[1][0] * A[2][2]; C[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0]; C[1][2] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    C[2][0] = A[1][0] * A[2][1] - A[1][1] * A[2][0]; C[2][1] = A[0][1] * A[2][0] - A[0][0] * A[2][1]; C[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    const double det = A[0][0] * C[0][0] + A[0][1] * C[1][0] + A[0][2] * C[2][0];
    bool   ok = det != 0.0 && std::isfinite(det);
    double norm_a = 0.0, norm_i = 0.0, extent = 0.0;
    for (int q = 0; q < 3; q++)
    {
        double ra = 0.0, ri = 0.0;
        for (int c = 0; c < 3; c++)
        {
            const double v = ok ? C[q][c] / det : 0.0;
            inv[c * 3 + q] = (float)v;
            ok = ok && std::isfinite(inv[c * 3 + q]);
            ra += std::fabs(A[q][c]); ri += std::fabs(v);
            extent += std::fabs(A[q][c]) * (double)am[c];
        }
        iar[q] = (float)(ri * (1.0 + 1e-6));
        extent += std::fabs((double)m[12 + q]);
        norm_a = std::max(norm_a, ra); norm_i = std::max(norm_i, ri);
    }
    *extent_out = (float)(extent * (1.0 + 1e-6));
    ok = ok && std::isfinite(*extent_out) && std::isfinite(iar[0]) && std::isfinite(iar[1]) && std::isfinite(iar[2]) && norm_a * norm_i <= 1e7;
    *flags = 0u;
    if (!ok)
    {
        for (int q = 0; q < 9; q++) inv[q] = 0.0f;
        iar[0] = iar[1] = iar[2] = 0.0f; *extent_out = 0.0f; *flags = 1u;
    }
}

static void ref_box(const float* m, const float* mb, float* box)
{
    double l[3] = { 1e300, 1e300, 1e300 }, h[3] = { -1e300, -1e300, -1e300 };
    if (mb[0] <= mb[3])
        for (int c = 0; c < 8; c++)
        {
            const double x = mb[(c & 1) ? 3 : 0], y = mb[(c & 2) ? 4 : 1], z = mb[(c & 4) ? 5 : 2];
            for (int k = 0; k < 3; k++)
            {
                const double v = (double)m[k] * x + (double)m[4 + k] * y + (double)m[8 + k] * z + (double)m[12 + k];
                const double e = 1e-6 * (std::fabs((double)m[k] * x) + std::fabs((double)m[4 + k] * y) + std::fabs((double)m[8 + k] * z) + std::fabs((double)m[12 + k]));
                l[k] = std::min(l[k], v - e); h[k] = std::max(h[k], v + e);
            }
        }
    else
        for (int k = 0; k < 3; k++) { l[k] = h[k] = (double)m[12 + k]; }
    for (int k = 0; k < 3; k++)
    {
        float lo = (float)l[k], hi = (float)h[k];
        if ((double)lo > l[k]) lo = std::nextafter(lo, -INFINITY);
        if ((double)hi < h[k]) hi = std::nextafter(hi, INFINITY);
        box[k] = lo; box[3 + k] = hi;
    }
}

static void matrix(float* m, float sx, float sy, float sz, float tx, float ty, float tz, float angle)
{
    const float c = std::cos(angle), s = std::sin(angle);
    const float r[16] = { c * sx, 0, -s * sx, 0, 0, sy, 0, 0, s * sz, 0, c * sz, 0, tx, ty, tz, 1 };   // about y, column-major
    std::memcpy(m, r, 64);
}

static std::vector<float> hostile_matrices()
{
    std::vector<float> out;
    auto push = [&](const float* m) { out.insert(out.end(), m, m + 16); };
    float m[16];
    matrix(m, 1, 1, 1, 0, 0, 0, 0.0f); push(m);
    matrix(m, 20, 0, 20, 30, 20, 60, 0.4f); push(m);                      // squashed to a plane
    matrix(m, 0, 0, 0, 70, 20, 30, 0.0f); push(m);                        // a point
    matrix(m, 15, 15, 15, 4000, 3000, -2500, 1.1f); push(m);              // far away
    matrix(m, -12, 9, 14, 60, 30, 40, 0.7f); push(m);                     // mirrored
    matrix(m, 1e-4f, 1e-4f, 1e-4f, 45, 70, 70, 0.3f); push(m);            // tiny
    matrix(m, 1e4f, 1e4f, 1e4f, 0, 0, 0, 0.2f); push(m);                  // huge
    matrix(m, 12, 12, 12, 75, 60, 20, 0.0f); m[4] = 9.0f; m[9] = -7.0f; push(m);   // a shear
    for (float eps : { 2e-5f, 2.2e-6f, 1.8e-6f })                         // condition about 1e6, 9e6 and 1.1e7
    {
        matrix(m, 1, 1, 1, 40, 40, 55, 0.0f);
        m[0] = 10; m[1] = 0; m[2] = 0; m[4] = 10; m[5] = eps; m[6] = 0; m[8] = 0; m[9] = 0; m[10] = 10;
        push(m);
    }
    matrix(m, 3e38f, 3e38f, 3e38f, 0, 0, 0, 0.0f); push(m);              // the extent and the box overflow
    matrix(m, 1e-30f, 1e-30f, 1e-30f, 1, 2, 3, 0.0f); push(m);           // the determinant underflows
    for (int i = 0; i < 2000; i++)
    {
        matrix(m, uni(-30, 30), uni(-30, 30), uni(-30, 30), uni(-500, 500), uni(-500, 500), uni(-500, 500), uni(0, 6.28f));
        m[4] = uni(-3, 3); m[6] = uni(-3, 3);
        push(m);
    }
    return out;
}

// ---- 3: a top level of n instances, breadth-first slots as instances_shared.hip build_shared_top lays them out -----------------------------------
struct Top { std::vector<SharedTopNode> nodes; std::vector<int> leaf_inst; int max_depth = 0; };

static Top make_top(int n)
{
    Top t;
    struct Q { int first, count, depth; };
    std::vector<Q> queue { { 0, n, 0 } };
    for (size_t qi = 0; qi < queue.size(); qi++)
    {
        const Q q = queue[qi];
        SharedTopNode nd { 0, 0, (int)queue.size(), (int)t.leaf_inst.size(), (int)(rnd() % 3), q.depth };
        const int parts = q.count <= 8 ? q.count : 2 + (int)(rnd() % 7);
        std::vector<Q> internal;
        int at = q.first;
        for (int p = 0; p < parts; p++)
        {
            int c = q.count <= 8 ? 1 : (p + 1 == parts ? q.first + q.count - at : std::max(1, std::min(q.first + q.count - at - (parts - 1 - p), (int)(rnd() % (2 * q.count / parts + 1)))));
            if (c == 1) { t.leaf_inst.push_back(at); nd.n_leaves++; }
            else internal.push_back({ at, c, q.depth + 1 });
            at += c;
        }
        nd.n_internal = (int)internal.size();
        for (const Q& c : internal) queue.push_back(c);
        if (!internal.empty()) t.max_depth = std::max(t.max_depth, q.depth + 1);
        t.nodes.push_back(nd);
    }
    return t;
}

static double refit_slot(const Top& t, int slot, const std::vector<float>& inst_box, float pad, std::vector<float>& box, std::vector<Node8>& out)
{
    const SharedTopNode& n = t.nodes[(size_t)slot];
    const int nc = n.n_internal + n.n_leaves;
    float clo[8][3], chi[8][3], lo[3], hi[3];
    for (int c = 0; c < nc; c++)
        for (int k = 0; k < 3; k++)
        {
            if (c < n.n_internal) { clo[c][k] = box[((size_t)n.child_base + c) * 6 + k]; chi[c][k] = box[((size_t)n.child_base + c) * 6 + 3 + k]; }
            else
            {
                const float* b = &inst_box[(size_t)t.leaf_inst[(size_t)n.leaf_base + (c - n.n_internal)] * 6];
                clo[c][k] = b[k] - pad; chi[c][k] = b[3 + k] + pad;
            }
        }
    const double area = imath::top_node(n, clo, chi, out[(size_t)slot], lo, hi);
    for (int k = 0; k < 3; k++) { box[(size_t)slot * 6 + k] = lo[k]; box[(size_t)slot * 6 + 3 + k] = hi[k]; }
    return area;
}

// the node body as instances_shared.hip refit_shared_top had it before it called the header: <cmath> calls, std::min / std::max
static uint8_t ref_exponent(float extent)
{
    if (!(extent > 0.0f)) return 1;
    int ex;
    (void)std::frexp(extent / 255.0f, &ex);
    int e = ex + 127;
    if (e < 1) e = 1;
    if (e > 254) e = 254;
    while (e > 1 && std::ldexp(255.0, e - 1 - 127) >= (double)extent) e--;
    while (e < 254 && std::ldexp(255.0, e - 127) < (double)extent) e++;
    return (uint8_t)e;
}

static double ref_node(const SharedTopNode& t, const float (*clo)[3], const float (*chi)[3], Node8& nd)
{
    const int nc = t.n_internal + t.n_leaves;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int c = 0; c < nc; c++)
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], clo[c][k]); hi[k] = std::max(hi[k], chi[c][k]); }
    std::memset(&nd, 0, sizeof(nd));
    nd.ox = lo[0]; nd.oy = lo[1]; nd.oz = lo[2];
    nd.ex = ref_exponent(hi[0] - lo[0]); nd.ey = ref_exponent(hi[1] - lo[1]); nd.ez = ref_exponent(hi[2] - lo[2]);
    nd.counts = (uint8_t)(t.n_internal | (nc << 4));
    nd.child_base = (uint32_t)t.child_base;
    nd.tri_base = (uint32_t)t.leaf_base;
    const uint8_t eb[3] = { nd.ex, nd.ey, nd.ez };
    for (int c = 0; c < nc; c++)
    {
        nd.meta[c] = c < t.n_internal ? (uint8_t)(0x10 | (c == 0 ? t.axis : 0)) : (uint8_t)((1 << 5) | (c - t.n_internal));
        for (int k = 0; k < 3; k++)
        {
            const double sc = std::ldexp(1.0, (int)eb[k] - 127), o = (double)lo[k];
            double l = std::floor(((double)clo[c][k] - o) / sc), h = std::ceil(((double)chi[c][k] - o) / sc);
            if (!(l > 0.0)) l = 0.0;
            if (l > 255.0) l = 255.0;
            if (!(h < 255.0)) h = 255.0;
            if (h < l) h = l;
            nd.qlo[k][c] = (uint8_t)l; nd.qhi[k][c] = (uint8_t)h;
        }
    }
    const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
    return x * y + y * z + z * x;
}

int main()
{
    // 1
    const float edge[] = { 0.0f, -0.0f, 1.0f, -1.0f, 1.17549435e-38f, -1.17549435e-38f, 1.4e-45f, -1.4e-45f, 3.4028235e38f, -3.4028235e38f, INFINITY, -INFINITY, 16777216.0f, 0.1f, -0.1f };
    std::vector<float> vals(edge, edge + sizeof(edge) / sizeof(edge[0]));
    for (int i = 0; i < 20000; i++) { uint32_t u = (rnd() << 8) ^ rnd(); float f; std::memcpy(&f, &u, 4); if (f == f) vals.push_back(f); }
    for (size_t i = 0; i < vals.size(); i++)
    {
        const float d = imath::next_down(vals[i]), u = imath::next_up(vals[i]), rd = std::nextafter(vals[i], -INFINITY), ru = std::nextafter(vals[i], INFINITY);
        if (std::memcmp(&d, &rd, 4) || std::memcmp(&u, &ru, 4)) return fail("next_down / next_up", (int)i);
        if (imath::finite_f(vals[i]) != (bool)std::isfinite(vals[i])) return fail("finite_f", (int)i);
        const float ext = std::fabs(vals[i]);
        int want = 1;   // the definition: smallest e in [1, 254] with ext <= 255 * 2^(e - 127)
        if (ext > 0.0f) while (want < 254 && std::ldexp(255.0, want - 127) < (double)ext) want++;
        if (imath::exponent_for(ext) != want) return fail("exponent_for", (int)i);
    }
    std::printf("helpers: %zu values equal <cmath>\n", vals.size());

    // 2
    const std::vector<float> mats = hostile_matrices();
    const int n_mats = (int)(mats.size() / 16);
    const float bounds[3][6] = { { -1, -1, -1, 1, 1, 1 }, { 0, -0.5f, 2, 3, 0.25f, 2 }, { 1, 0, 0, 0, 0, 0 } };   // a cube, a flat one, an empty mesh (lo > hi)
    int flagged = 0;
    for (int i = 0; i < n_mats; i++)
        for (int b = 0; b < 3; b++)
        {
            const float* m = &mats[(size_t)i * 16];
            float am[3];
            for (int k = 0; k < 3; k++) am[k] = b == 2 ? 0.0f : std::max(std::fabs(bounds[b][k]), std::fabs(bounds[b][3 + k]));
            float inv[9], iar[3], ext, rinv[9], riar[3], rext, box[6], rbox[6];
            uint32_t fl, rfl;
            imath::record_terms(m, am, inv, iar, &ext, &fl);
            ref_record(m, am, rinv, riar, &rext, &rfl);
            if (std::memcmp(inv, rinv, 36) || std::memcmp(iar, riar, 12) || std::memcmp(&ext, &rext, 4) || fl != rfl) return fail("record_terms", i);
            imath::world_box(m, bounds[b], box);
            ref_box(m, bounds[b], rbox);
            if (std::memcmp(box, rbox, 24)) return fail("world_box", i);
            flagged += b == 0 && fl;
        }
    if (flagged < 4) return fail("hostile matrices that switch culling off", flagged);
    std::printf("records and boxes: %d matrices x 3 meshes equal the <cmath> restatement, %d flagged\n", n_mats, flagged);

    // 3
    const int I = 601;
    const Top t = make_top(I);
    if ((int)t.leaf_inst.size() != I) return fail("make_top leaves", (int)t.leaf_inst.size());
    std::vector<float> inst_box((size_t)I * 6);
    for (int i = 0; i < I; i++)
    {
        float m[16];
        matrix(m, uni(2, 20), uni(2, 20), uni(2, 20), uni(0, 100), uni(0, 100), uni(0, 100), uni(0, 6.28f));
        imath::world_box(m, bounds[0], &inst_box[(size_t)i * 6]);
    }
    const float glo[3] = { -30, -30, -30 }, ghi[3] = { 130, 130, 130 };
    const float pad = imath::pad_of_bounds(glo, ghi);
    const size_t N = t.nodes.size();
    std::vector<Node8> by_slot(N), by_depth(N);
    std::vector<float> box_a(N * 6), box_b(N * 6, NAN);   // a depth-ordered refit that read a slot too early would read NaN
    std::vector<double> area_a(N), area_b(N);
    for (size_t slot = N; slot-- > 0;) area_a[slot] = refit_slot(t, (int)slot, inst_box, pad, box_a, by_slot);
    std::vector<int> start;
    for (size_t j = 0; j < N; j++)
    {
        if (t.nodes[j].depth == (int)start.size()) start.push_back((int)j);
        else if (t.nodes[j].depth != (int)start.size() - 1) return fail("slots in depth order", (int)j);
    }
    start.push_back((int)N);
    for (int d = (int)start.size() - 2; d >= 0; d--)
        for (int j = start[(size_t)d]; j < start[(size_t)d + 1]; j++) area_b[(size_t)j] = refit_slot(t, j, inst_box, pad, box_b, by_depth);
    if (std::memcmp(by_slot.data(), by_depth.data(), N * sizeof(Node8)) || std::memcmp(box_a.data(), box_b.data(), N * 24) || std::memcmp(area_a.data(), area_b.data(), N * 8))
        return fail("depth-by-depth refit against slot order", 0);
    for (size_t j = 0; j < N; j++)   // the header's node against the <cmath> restatement, over the boxes the refit above left
    {
        const SharedTopNode& n = t.nodes[j];
        const int nc = n.n_internal + n.n_leaves;
        float clo[8][3], chi[8][3];
        for (int c = 0; c < nc; c++)
            for (int k = 0; k < 3; k++)
            {
                if (c < n.n_internal) { clo[c][k] = box_a[((size_t)n.child_base + c) * 6 + k]; chi[c][k] = box_a[((size_t)n.child_base + c) * 6 + 3 + k]; }
                else { const float* b = &inst_box[(size_t)t.leaf_inst[(size_t)n.leaf_base + (c - n.n_internal)] * 6]; clo[c][k] = b[k] - pad; chi[c][k] = b[3 + k] + pad; }
            }
        Node8 ref;
        const double ra = ref_node(n, clo, chi, ref);
        if (std::memcmp(&ref, &by_slot[j], sizeof(Node8)) || std::memcmp(&ra, &area_a[j], 8)) return fail("top_node against the <cmath> restatement", (int)j);
    }
    {   // and over extents the room above never makes: flat, tiny, huge and overflowing nodes
        const float ext[] = { 0.0f, 1e-30f, 1e-7f, 255.0f, 255.00002f, 256.0f, 1e20f, 3e38f };
        for (size_t i = 0; i < sizeof(ext) / sizeof(ext[0]); i++)
        {
            const SharedTopNode n { 1, 2, 1, 0, (int)(i % 3), 0 };
            const float clo[8][3] = { { -ext[i], 0.0f, 1.0f }, { 0.25f * ext[i], -1.0f, 1.0f }, { -ext[i], -ext[i], -ext[i] } };
            const float chi[8][3] = { { ext[i], 0.0f, 2.0f }, { 0.5f * ext[i], 1.0f, 1.0f + ext[i] }, { -0.5f * ext[i], ext[i], ext[i] } };
            Node8 ref, got;
            float lo[3], hi[3];
            const double ra = ref_node(n, clo, chi, ref), ga = imath::top_node(n, clo, chi, got, lo, hi);
            if (std::memcmp(&ref, &got, sizeof(Node8)) || std::memcmp(&ra, &ga, 8)) return fail("top_node over extreme extents", (int)i);
        }
    }
    for (size_t j = 0; j < N; j++)   // every child box lies inside its quantised slot
    {
        const Node8& nd = by_slot[j];
        if ((nd.counts & 15) != t.nodes[j].n_internal || (nd.counts >> 4) != t.nodes[j].n_internal + t.nodes[j].n_leaves) return fail("counts", (int)j);
        const float o[3] = { nd.ox, nd.oy, nd.oz };
        const uint8_t e[3] = { nd.ex, nd.ey, nd.ez };
        for (int c = 0; c < (nd.counts & 15); c++)
            for (int k = 0; k < 3; k++)
            {
                const double sc = std::ldexp(1.0, (int)e[k] - 127);
                const float* cb = &box_a[((size_t)nd.child_base + c) * 6];
                if ((double)o[k] + nd.qlo[k][c] * sc > (double)cb[k] || (double)o[k] + nd.qhi[k][c] * sc < (double)cb[3 + k]) return fail("a quantised child box is not conservative", (int)j);
            }
    }
    std::printf("top level: %zu nodes over %d instances, %zu depths: depth order equals slot order\n", N, I, start.size() - 1);
    return 0;
}
