// The refit of split-free trees under new vertices: the engine of hr_scene_update_vertices (deform.hip: a flat scene is ONE flagged mesh with root 0)
// and hr_scene_update_meshes (instances_shared_deform.hip: the flagged meshes of a shared instanced scene).  A flagged mesh is built without
// spatial splits, so every finite triangle has ONE reference and a leaf's box is the bounds of its finite triangles plus the builder's pad for the mesh's current bounds:
// a refit needs no cells (instances.hip needs them because its trees are split).
//
// An update, all on the caller's stream, in this order (entries are taken kMaxUpdatesPerLaunch at a time):
//   k_deform_scatter     one launch for all entries: one thread per updated triangle writes the 36 vertex bytes of its reference (through the
//                        triangle -> reference map; prim and the padding words stand), its positions row and, when given, its normals row
//   k_deform_bounds      one launch for all updated meshes: the exact bounds of every mesh's finite references, by one atomic pair per axis per
//                        workgroup (of up to 64 a mesh) into the mesh's six words of bounds_bits — what the builder computes before it pads (bvh_build.cpp), so that the
//                        refit pads for the size the mesh has NOW (refit.h refit_pad).  The words stand at 0xffffffff / 0 between updates: the
//                        mesh's workgroup of k_deform_refit_top, their last reader, puts them back.
//   k_deform_refit       refit.h refit_node<false>, level d of ALL updated meshes in one launch, deepest level first: the launch count follows the
//                        deepest updated mesh, not the number of meshes.  Only levels wider than the mesh's narrow width come here.
//   k_deform_refit_top   one launch, one workgroup per updated mesh: the narrow levels near its root, a barrier between levels, then the refitted
//                        root box to root_box[mesh] and, when the caller gave bounds, whether they contain it to outside[mesh] (plain vector stores)
// Launch boundaries and workgroup barriers are the only ordering between levels: the per-XCD L2s are not coherent with each other (see the header
// of instances.hip).  Every node of an updated mesh is refitted, whatever the updated range: a parent's box depends on all its leaves.
// The refit cost (sum of the nodes' half areas now / when built — the measure the instanced scenes' top-level re-build trigger uses,
// top_area_at_build) rides in the refit: every workgroup reduces its nodes' areas (double, a fixed butterfly) and stores ONE partial sum in its own
// slot with a plain vector store — slot 0 of a mesh belongs to its one-workgroup launch, the wide levels follow, deepest first — and the host adds
// a mesh's slots in index order when the ratio is asked for.  No atomic: a sum in arrival order would not reproduce, and "the same vertices give
// exactly 1.0" is a test of the refit's encoding.
#include "deform_refit.h"
#include "refit.h"
#include <algorithm>
#include <cstring>

using namespace hr;

namespace {

constexpr int kLevelStride = kMaxTraversalDepth + 2;
constexpr int kTopOffsets = 192;    // level offsets one one-workgroup launch carries: three per mesh at 64 meshes; a launch takes fewer meshes when they need more

// Everything a kernel needs to find its work travels in its arguments (the host holds the level rows): a table in device memory would put one
// more dependent load in front of every launch's first node.
struct ScatterEntry { const float* positions; const float* normals; uint32_t first; int32_t count, block_first; };   // first: in the attribute arrays
struct ScatterArgs
{
    TriGPU*        tris;
    const int32_t* tri_ref;
    float*         positions;
    float*         normals;     // or null
    int            n;
    ScatterEntry   e[kMaxUpdatesPerLaunch];
};

__global__ __launch_bounds__(256) void k_deform_scatter(ScatterArgs a)
{
    int j = 0;
    for (int i = 1; i < a.n; i++) if ((int)blockIdx.x >= a.e[i].block_first) j = i;
    const ScatterEntry& e = a.e[j];
    const int t = ((int)blockIdx.x - e.block_first) * 256 + (int)threadIdx.x;
    if (t >= e.count) return;
    const size_t g = (size_t)e.first + t;
    const float* p = e.positions + (size_t)t * 9;
    float v[9];
    for (int k = 0; k < 9; k++) v[k] = p[k];
    float* w = a.positions + g * 9;
    for (int k = 0; k < 9; k++) w[k] = v[k];
    const int32_t r = a.tri_ref[g];
    if (r >= 0)
    {
        TriGPU& d = a.tris[r];   // prim and the padding words stand
        d.v0[0] = v[0]; d.v0[1] = v[1]; d.v0[2] = v[2];
        d.v1[0] = v[3]; d.v1[1] = v[4]; d.v1[2] = v[5];
        d.v2[0] = v[6]; d.v2[1] = v[7]; d.v2[2] = v[8];
    }
    if (e.normals)
    {
        const float* n = e.normals + (size_t)t * 9;
        float*       o = a.normals + g * 9;
        for (int k = 0; k < 9; k++) o[k] = n[k];
    }
}

struct BoundsEntry { uint32_t first, mesh; int32_t count, block_first, blocks; };   // the mesh's references in `tris`, its workgroups in this launch
struct BoundsArgs
{
    const TriGPU* tris;
    uint32_t*     bits;
    int           n;
    BoundsEntry   e[kMaxUpdatesPerLaunch];
};
constexpr int kBoundsPerBlock = 1024, kBoundsMaxBlocks = 64;   // references a workgroup takes before a mesh gets another one; workgroups per mesh at most

// Atomics of all workgroups on the same six words serialise across the XCDs (one per wave cost a 20 k-triangle mesh more than its whole refit): a
// workgroup strides over its share, reduces in registers, then through LDS, and issues ONE pair per axis.
__global__ __launch_bounds__(256) void k_deform_bounds(BoundsArgs a)
{
    __shared__ float s_lo[4][3], s_hi[4][3];
    int j = 0;
    for (int i = 1; i < a.n; i++) if ((int)blockIdx.x >= a.e[i].block_first) j = i;
    const BoundsEntry& e = a.e[j];
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int t = ((int)blockIdx.x - e.block_first) * 256 + (int)threadIdx.x; t < e.count; t += e.blocks * 256)
    {
        const uint4* p = reinterpret_cast<const uint4*>(a.tris + (size_t)e.first + t);   // three 16-byte loads (traverse.h load_tri)
        const uint4  q0 = p[0], q1 = p[1], q2 = p[2];
        const float  v[3][3] = { { __uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z) }, { __uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z) },
                                 { __uint_as_float(q2.x), __uint_as_float(q2.y), __uint_as_float(q2.z) } };
        bool fin = true;
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) fin = fin && fabsf(v[i][k]) < INFINITY;
        for (int k = 0; k < 3; k++)
        {
            lo[k] = fminf(lo[k], fin ? fminf(v[0][k], fminf(v[1][k], v[2][k])) : INFINITY);
            hi[k] = fmaxf(hi[k], fin ? fmaxf(v[0][k], fmaxf(v[1][k], v[2][k])) : -INFINITY);
        }
    }
    for (int k = 0; k < 3; k++)
    {
        float l = lo[k], h = hi[k];
        for (int o = 32; o > 0; o >>= 1) { l = fminf(l, __shfl_xor(l, o)); h = fmaxf(h, __shfl_xor(h, o)); }
        if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6][k] = l; s_hi[threadIdx.x >> 6][k] = h; }
    }
    __syncthreads();
    if (threadIdx.x < 3)
    {
        const int   k = (int)threadIdx.x;
        const float l = fminf(fminf(s_lo[0][k], s_lo[1][k]), fminf(s_lo[2][k], s_lo[3][k])), h = fmaxf(fmaxf(s_hi[0][k], s_hi[1][k]), fmaxf(s_hi[2][k], s_hi[3][k]));
        uint32_t*   bits = a.bits + (size_t)e.mesh * 6;
        if (l <= h) { atomicMin(bits + k, ordered_bits(l)); atomicMax(bits + 3 + k, ordered_bits(h)); }
    }
}

struct LevelEntry { int32_t first, end, slot, block_first; uint32_t mesh; };   // the level's range in `lists`, its first partial slot, the mesh
struct LevelArgs
{
    RefitArgs       r;          // list / count / pad unused: they differ per mesh
    const uint32_t* bits;       // bounds_bits of all meshes
    const uint32_t* lists;
    double*         partials;
    int             n;
    LevelEntry      e[kMaxUpdatesPerLaunch];
};

__global__ __launch_bounds__(64) void k_deform_refit(LevelArgs a)
{
    int j = 0;
    for (int i = 1; i < a.n; i++) if ((int)blockIdx.x >= a.e[i].block_first) j = i;
    const LevelEntry& e = a.e[j];
    const int local = (int)blockIdx.x - e.block_first;
    const int i     = e.first + local * 64 + (int)threadIdx.x;
    double area = 0.0;
    if (i < e.end)
    {
        RefitArgs r = a.r;
        r.pad = refit_pad(a.bits + (size_t)e.mesh * 6);
        area = refit_node<false>(r, a.lists[i]);
    }
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if (threadIdx.x == 0) a.partials[e.slot + local] = area;
}

struct TopEntry
{
    uint32_t mesh, root;
    int32_t  slot;
    int16_t  d_top;
    uint16_t offs_at;                // offs[offs_at + d] .. offs[offs_at + d + 1]: level d in `lists`
    uint32_t has_bounds;
    float    bounds[6];
};
struct TopArgs
{
    RefitArgs       r;
    uint32_t*       bits;       // bounds_bits of all meshes
    const uint32_t* lists;
    double*         partials;
    float*          root_box;
    uint32_t*       outside;
    int             n, n_offs;
    TopEntry        e[kMaxUpdatesPerLaunch];
    int32_t         offs[kTopOffsets];
};
static_assert(sizeof(TopArgs) <= 4096, "kernel arguments are limited to 4 KiB");
static_assert(kLevelStride <= kTopOffsets, "one mesh's narrow levels must fit one launch");

__global__ __launch_bounds__(256) void k_deform_refit_top(TopArgs t)
{
    __shared__ double s_sum[4];
    const TopEntry& e   = t.e[blockIdx.x];
    const int32_t*  row = t.offs + e.offs_at;
    RefitArgs r = t.r;
    uint32_t* bits = t.bits + (size_t)e.mesh * 6;
    r.pad = refit_pad(bits);
    double area = 0.0;
    for (int d = e.d_top; d >= 0; d--)
    {
        for (int i = row[d] + (int)threadIdx.x; i < row[d + 1]; i += 256) area += refit_node<false>(r, t.lists[i]);
        __threadfence_block();
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = area;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        t.partials[e.slot] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);   // also with d_top = -1: it clears slot 0
        const float* nb = r.node_box + (size_t)e.root * 8;
        float b[8];
        for (int k = 0; k < 8; k++) { b[k] = nb[k]; t.root_box[(size_t)e.mesh * 8 + k] = b[k]; }
        uint32_t out = 0u;
        if (e.has_bounds)
        {
            // the root box is the union of leaf boxes, each its triangles' bounds -/+ the pad in fp32: bounds that hold every vertex pass the
            // same subtraction / addition, which is monotonic, so exact bounds are never reported
            // (an empty root box, +inf / -inf, lies inside any bounds)
            const float pad = r.pad;
            for (int k = 0; k < 3; k++)
                if (b[k] <= b[4 + k] && (!(b[k] >= e.bounds[k] - pad) || !(b[4 + k] <= e.bounds[3 + k] + pad))) out = 1u;
        }
        t.outside[e.mesh] = out;
        for (int k = 0; k < 3; k++) { bits[k] = 0xffffffffu; bits[3 + k] = 0u; }   // every reader of this update is done (the barrier above)
    }
}

hr_status read_partials(const DeformRefit& sd, uint32_t m, double* sum)
{
    std::vector<double> part((size_t)sd.n_partials[m]);
    HR_HIP(hipMemcpy(part.data(), (const double*)sd.partials.p + sd.partial_base[m], part.size() * 8, hipMemcpyDeviceToHost));
    double a = 0.0;
    for (double v : part) a += v;
    *sum = a;
    return HR_OK;
}

// the exact bounds of the finite references of ms[0 .. n) into their words of bounds_bits (idle before)
void bounds_enqueue(hr_scene* s, const DeformRefit& sd, const uint32_t* ms, int n, hipStream_t st)
{
    BoundsArgs b;
    b.tris = (const TriGPU*)s->tris.p; b.bits = (uint32_t*)sd.bounds_bits.p; b.n = 0;
    int blocks = 0;
    for (int j = 0; j < n; j++)
    {
        if (sd.n_refs[ms[j]] == 0) continue;
        const int mine = std::min(kBoundsMaxBlocks, cdiv(sd.n_refs[ms[j]], kBoundsPerBlock));
        b.e[b.n++] = { sd.ref_base[ms[j]], ms[j], sd.n_refs[ms[j]], blocks, mine };
        blocks += mine;
    }
    if (b.n > 0) hipLaunchKernelGGL(k_deform_bounds, dim3(blocks), dim3(256), 0, st, b);
}

// the refit of the flagged meshes ms[0 .. n) of `sd` into `nodes` and `node_box`
hr_status enqueue(hr_scene* s, DeformRefit& sd, Node8* nodes, float* node_box, const uint32_t* ms, int n, const float* const* bounds, hipStream_t st)
{
    RefitArgs r;
    r.nodes = nodes; r.tris = (const TriGPU*)s->tris.p; r.node_box = node_box; r.pad = 0.0f;
    bounds_enqueue(s, sd, ms, n, st);
    r.cells = nullptr; r.node_inst = nullptr; r.inst = nullptr; r.dirty = nullptr; r.list = nullptr; r.count = 0;
    int deepest = 0;
    for (int j = 0; j < n; j++) deepest = std::max(deepest, sd.n_levels[ms[j]]);
    for (int d = deepest - 1; d >= 0; d--)
    {
        LevelArgs a;
        a.r = r; a.bits = (const uint32_t*)sd.bounds_bits.p; a.lists = (const uint32_t*)sd.level_nodes.p; a.partials = (double*)sd.partials.p; a.n = 0;
        int blocks = 0;
        for (int j = 0; j < n; j++)
        {
            const uint32_t m = ms[j];
            if (d >= sd.n_levels[m] || d <= sd.d_top[m]) continue;
            const int32_t* row = &sd.levels_host[(size_t)m * 2 * kLevelStride];
            if (row[d + 1] <= row[d]) continue;
            a.e[a.n++] = { row[d], row[d + 1], sd.partial_base[m] + row[kLevelStride + d], blocks, m };
            blocks += cdiv(row[d + 1] - row[d], 64);
        }
        if (a.n == 0) continue;
        hipLaunchKernelGGL(k_deform_refit, dim3(blocks), dim3(64), 0, st, a);
        sd.level_launches++;
    }
    TopArgs t;
    t.r = r; t.bits = (uint32_t*)sd.bounds_bits.p; t.lists = (const uint32_t*)sd.level_nodes.p; t.partials = (double*)sd.partials.p; t.root_box = (float*)sd.root_box.p; t.outside = (uint32_t*)sd.outside.p;
    t.n = t.n_offs = 0;
    for (int j = 0; j <= n; j++)
    {
        const int need = j < n ? sd.d_top[ms[j]] + 2 : 0;
        if (t.n > 0 && (j == n || t.n_offs + need > kTopOffsets))   // all n meshes in one launch unless their narrow levels outnumber the offsets it carries
        {
            hipLaunchKernelGGL(k_deform_refit_top, dim3((unsigned)t.n), dim3(256), 0, st, t);
            sd.top_launches++;
            t.n = t.n_offs = 0;
        }
        if (j == n) break;
        const uint32_t m = ms[j];
        TopEntry& e = t.e[t.n++];
        e.mesh = m; e.root = sd.root[m]; e.slot = sd.partial_base[m]; e.d_top = (int16_t)sd.d_top[m]; e.offs_at = (uint16_t)t.n_offs;
        e.has_bounds = bounds && bounds[j] ? 1u : 0u;
        if (e.has_bounds) std::memcpy(e.bounds, bounds[j], 24); else std::memset(e.bounds, 0, 24);
        std::memcpy(t.offs + t.n_offs, &sd.levels_host[(size_t)m * 2 * kLevelStride], (size_t)need * 4);
        t.n_offs += need;
    }
    HR_HIP(hipGetLastError());
    return HR_OK;
}

} // namespace

void hr::deform_refit_scatter(hr_scene* s, const DeformScatterEntry* e, int n, float* dst_positions, float* dst_normals, hipStream_t st)
{
    const DeformRefit& sd = *s->deform;
    ScatterArgs a;
    a.tris = (TriGPU*)s->tris.p; a.tri_ref = (const int32_t*)sd.tri_ref.p; a.positions = dst_positions; a.normals = dst_normals; a.n = n;
    int blocks = 0;
    for (int j = 0; j < n; j++)
    {
        a.e[j] = { e[j].positions, e[j].normals, sd.tri_base[e[j].mesh] + (uint32_t)e[j].first, e[j].count, blocks };
        blocks += cdiv(e[j].count, 256);
    }
    hipLaunchKernelGGL(k_deform_scatter, dim3(blocks), dim3(256), 0, st, a);
}

hr_status hr::deform_refit_enqueue(hr_scene* s, Node8* nodes, const uint32_t* ms, int n, const float* const* bounds, hipStream_t st)
{
    return enqueue(s, *s->deform, nodes, (float*)s->node_box.p, ms, n, bounds, st);
}

void hr::deform_refit_bounds_enqueue(hr_scene* s, const uint32_t* ms, int n, hipStream_t st) { bounds_enqueue(s, *s->deform, ms, n, st); }

hr_status hr::deform_refit_cost(hr_scene* s, uint32_t m, float* ratio)
{
    DeformRefit& sd = *s->deform;
    if (!sd.cost_known[m])
    {
        double now = 0.0;
        const hr_status e = read_partials(sd, m, &now);
        if (e != HR_OK) return e;
        sd.cost_ratio[m] = sd.cost_at_build[m] > 0.0 ? now / sd.cost_at_build[m] : 1.0;
        sd.cost_known[m] = 1;
    }
    *ratio = (float)sd.cost_ratio[m];
    return HR_OK;
}

hr_status hr::deform_refit_adopt(hr_scene* s, const std::vector<DeformMesh>& meshes, const char* call)
{
    const size_t M = meshes.size();
    std::unique_ptr<DeformRefit> fresh(new DeformRefit());   // the scene takes it only when it stands complete: a failure leaves an earlier one in place
    DeformRefit& sd = *fresh;
    sd.flag.assign(M, 0); sd.root.assign(M, 0); sd.ref_base.assign(M, 0); sd.tri_base.assign(M, 0); sd.n_tris.assign(M, 0); sd.n_refs.assign(M, 0);
    sd.n_levels.assign(M, 0); sd.d_top.assign(M, -1); sd.partial_base.assign(M, 0); sd.n_partials.assign(M, 0);
    sd.cost_at_build.assign(M, 0.0); sd.cost_known.assign(M, 1); sd.cost_ratio.assign(M, 1.0); sd.redeal_ok.assign(M, 0);
    sd.levels_host.assign(M * 2 * kLevelStride, 0);
    size_t n_tris_all = 0;
    bool any = false;
    for (size_t k = 0; k < M; k++)
    {
        sd.flag[k] = meshes[k].flag ? 1 : 0; sd.root[k] = meshes[k].root; sd.ref_base[k] = meshes[k].ref_base; sd.tri_base[k] = meshes[k].tri_base;
        sd.n_tris[k] = meshes[k].n_tris; sd.n_refs[k] = meshes[k].flag ? (int32_t)meshes[k].bvh->tris.size() : 0;
        any = any || sd.flag[k];
        n_tris_all = std::max(n_tris_all, (size_t)meshes[k].tri_base + (size_t)meshes[k].n_tris);
    }
    if (!any) { s->deform = std::move(fresh); return HR_OK; }
    std::vector<uint32_t> level_nodes;
    std::vector<int32_t>  tri_ref(n_tris_all, -1);
    int partials = 0;
    for (size_t k = 0; k < M; k++)
    {
        if (!sd.flag[k]) continue;
        const BuiltBVH& b = *meshes[k].bvh;
        const size_t n_nodes = b.nodes.size();
        std::vector<int> depth(n_nodes, 0);   // children follow their parent in the builder's breadth-first order
        int max_depth = 0;
        for (size_t j = 0; j < n_nodes; j++)
            for (int c = 0; c < (b.nodes[j].counts & 15); c++) { depth[(size_t)b.nodes[j].child_base + c] = depth[j] + 1; max_depth = std::max(max_depth, depth[j] + 1); }
        const int n_levels = max_depth + 1;
        if (n_levels + 1 > kLevelStride) { set_last_error(std::string(call) + ": a mesh tree deeper than the traversal stack"); return HR_ERR_UNSUPPORTED; }
        int32_t* row = &sd.levels_host[k * 2 * kLevelStride];
        std::vector<int32_t> width((size_t)n_levels, 0);
        for (size_t j = 0; j < n_nodes; j++) width[(size_t)depth[j]]++;
        row[0] = (int32_t)level_nodes.size();
        for (int d = 0; d < n_levels; d++) row[d + 1] = row[d] + width[(size_t)d];
        level_nodes.resize((size_t)row[n_levels]);
        {
            std::vector<int32_t> cur(row, row + n_levels);
            for (size_t j = 0; j < n_nodes; j++) level_nodes[(size_t)cur[(size_t)depth[j]]++] = sd.root[k] + (uint32_t)j;   // global node indices
        }
        int d_top = -1;   // (the depth check above keeps d_top + 1 <= kMaxTraversalDepth, the rows' length)
        while (d_top + 1 < n_levels && width[(size_t)d_top + 1] <= meshes[k].narrow) d_top++;
        // slot 0: the one-workgroup launch; then the wide levels, deepest first
        int slot = 1;
        for (int d = n_levels - 1; d > d_top; d--) { row[kLevelStride + d] = slot; slot += cdiv(width[(size_t)d], 64); }
        sd.n_levels[k] = n_levels; sd.d_top[k] = d_top; sd.partial_base[k] = partials; sd.n_partials[k] = slot;
        partials += slot;
        {
            // the re-deal's table; a tree whose leaves do not name each reference once (no builder of this library makes one) cannot be re-dealt
            std::vector<int32_t> order(b.tris.size());
            int32_t n_order = 0;
            bool ok = deform_leaf_order(b.nodes.data(), (int32_t)n_nodes, 0u, order.data(), (int32_t)order.size(), &n_order) && (size_t)n_order == b.tris.size();
            std::vector<uint8_t> seen(b.tris.size(), 0);
            for (size_t r = 0; ok && r < order.size(); r++) { ok = order[r] >= 0 && (size_t)order[r] < seen.size() && !seen[(size_t)order[r]]; if (ok) seen[(size_t)order[r]] = 1; }
            sd.redeal_ok[k] = ok ? 1 : 0;
            if (sd.slot_of_rank_host.size() < (size_t)sd.ref_base[k] + b.tris.size()) sd.slot_of_rank_host.resize((size_t)sd.ref_base[k] + b.tris.size(), -1);
            for (size_t r = 0; ok && r < order.size(); r++) sd.slot_of_rank_host[(size_t)sd.ref_base[k] + r] = (int32_t)sd.ref_base[k] + order[r];
        }
        for (size_t r = 0; r < b.tris.size(); r++)
        {
            const uint32_t prim = b.tris[r].prim;
            if (prim >= (uint32_t)sd.n_tris[k] || tri_ref[(size_t)sd.tri_base[k] + prim] >= 0)
            {
                set_last_error(std::string(call) + ": a triangle with more than one reference in a tree built without spatial splits");
                return HR_ERR_UNSUPPORTED;
            }
            tri_ref[(size_t)sd.tri_base[k] + prim] = (int32_t)(sd.ref_base[k] + r);
        }
    }
    const size_t n_nodes_all = (size_t)s->info.n_nodes;
    hr_status e;
    if ((e = sd.level_nodes.alloc(level_nodes.size() * 4)) != HR_OK) return e;
    if ((e = sd.tri_ref.alloc(tri_ref.size() * 4)) != HR_OK) return e;
    if ((e = sd.partials.alloc((size_t)partials * 8)) != HR_OK) return e;
    if ((e = sd.root_box.alloc(M * 32)) != HR_OK) return e;
    if ((e = sd.outside.alloc(M * 4)) != HR_OK) return e;
    if ((e = sd.bounds_bits.alloc(M * 24)) != HR_OK) return e;
    {
        std::vector<uint32_t> idle(M * 6);
        for (size_t k = 0; k < M * 6; k++) idle[k] = k % 6 < 3 ? 0xffffffffu : 0u;
        HR_HIP(hipMemcpy(sd.bounds_bits.p, idle.data(), M * 24, hipMemcpyHostToDevice));
    }
    DevBuf node_box;
    if ((e = node_box.alloc(n_nodes_all * 32)) != HR_OK) return e;
    HR_HIP(hipHostMalloc((void**)&sd.root_box_host, M * 32, hipHostMallocDefault));
    std::memset(sd.root_box_host, 0, M * 32);
    HR_HIP(hipMemcpy(sd.level_nodes.p, level_nodes.data(), level_nodes.size() * 4, hipMemcpyHostToDevice));
    if (!tri_ref.empty()) HR_HIP(hipMemcpy(sd.tri_ref.p, tri_ref.data(), tri_ref.size() * 4, hipMemcpyHostToDevice));
    // one refit into a scratch copy of the nodes (the scene's own stay as built): node_box and the cost of every flagged tree as built
    DevBuf scratch;
    if ((e = scratch.alloc(n_nodes_all * sizeof(Node8))) != HR_OK) return e;
    HR_HIP(hipMemcpy(scratch.p, s->nodes.p, n_nodes_all * sizeof(Node8), hipMemcpyDeviceToDevice));
    std::vector<uint32_t> ms;
    for (size_t k = 0; k <= M; k++)
    {
        if (k < M && sd.flag[k]) ms.push_back((uint32_t)k);
        if (!ms.empty() && (k == M || ms.size() == (size_t)kMaxUpdatesPerLaunch))
        {
            if ((e = enqueue(s, sd, (Node8*)scratch.p, (float*)node_box.p, ms.data(), (int)ms.size(), nullptr, nullptr)) != HR_OK) return e;
            ms.clear();
        }
    }
    HR_HIP(hipStreamSynchronize(nullptr));
    for (size_t k = 0; k < M; k++)
        if (sd.flag[k] && (e = read_partials(sd, (uint32_t)k, &sd.cost_at_build[k])) != HR_OK) return e;
    sd.level_launches = sd.top_launches = 0;
    std::swap(s->node_box.p, node_box.p); std::swap(s->node_box.bytes, node_box.bytes);
    s->deform = std::move(fresh);
    return HR_OK;
}
