// The two device sorts of 64-bit (code, index) keys, shared by the top level's device re-build (instances_shared_rebuild.hip: instances by the
// Morton code of their world box) and the re-deal of a deformable mesh's triangles (deform_redeal.hip: triangles by the Morton code of their box).
//   * up to kSortSmall keys: a bitonic network in ONE workgroup's LDS (bitonic_sort_lds; the caller's kernel fills the keys and reads the order)
//   * above: a stable LSD radix sort of (code, index) over kRadixPasses 8-bit digits of the 32-bit code, which starts from ascending indices and
//     hence ends in the order of the 64-bit keys (radix_sort_enqueue: k_radix_hist / k_radix_scan / k_radix_scatter per digit)
// Every launch takes the status block and `predicated` of a predicated top-level re-build (exit at once unless the block's rebuild_flag is set);
// callers without one pass nullptr and 0.
//
// kSortSmall = 4096 keys: 4096 x 8 bytes = 32 KiB of LDS, half of the 64 KiB a workgroup gets without asking for more and a fifth of the 160 KiB
// a gfx950 workgroup may declare, at 1024 lanes (16 waves of 64) four keys per lane.  The network over n2 = 2^k >= n keys costs k (k + 1) / 2
// barriers — 78 at 4096 — against the 13 launches of the radix path, which is what a launch-latency-bound job of this size is decided by;
// doubling the limit would add 13 barriers and halve nothing.
#pragma once
#include "instances_shared_device.h"

namespace hr {
namespace {   // internal linkage on purpose: a kernel is launched from the translation unit that defines it (no relocatable device code in this build)

constexpr int kSortSmall  = 4096;
constexpr int kSortLanes  = 1024;
constexpr int kRadixBits  = 8, kRadixBins = 1 << kRadixBits, kRadixPasses = 4;   // 4 x 8 bits cover a 30-bit code and the bit above it
constexpr int kRadixTile  = 256;                                                  // one key per lane

__device__ inline bool rebuild_skipped(const DeviceUpdateStatus* st, int predicated) { return predicated && st->rebuild_flag == 0u; }

// key[0 .. n2) in LDS, ascending on return; n2 a power of two <= kSortSmall, every lane of a kSortLanes-wide workgroup calls it after a barrier
// behind the writes of the keys
__device__ inline void bitonic_sort_lds(unsigned long long* key, int n2, int t)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
        {
            for (int e = t; e < n2; e += kSortLanes)
            {
                const int p = e ^ j;
                if (p > e)
                {
                    const unsigned long long a = key[e], b = key[p];
                    const bool up = (e & k) == 0;
                    if ((a > b) == up) { key[e] = b; key[p] = a; }
                }
            }
            __syncthreads();
        }
}

// hist[digit * n_blocks + block]: keys of this workgroup's tile with that digit
__global__ void __launch_bounds__(kRadixTile) k_radix_hist(const uint32_t* codes, uint32_t* hist, const DeviceUpdateStatus* status, int n, int shift, int predicated)
{
    __shared__ uint32_t cnt[kRadixBins];
    if (rebuild_skipped(status, predicated)) return;
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int i = (int)(blockIdx.x * kRadixTile + threadIdx.x);
    if (i < n) atomicAdd(&cnt[(codes[i] >> shift) & (kRadixBins - 1)], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive prefix over hist in place (digit-major: all tiles of digit 0, then of digit 1, ...); one workgroup, every lane a contiguous chunk
__global__ void __launch_bounds__(kSortLanes) k_radix_scan(uint32_t* hist, const DeviceUpdateStatus* status, int total, int predicated)
{
    __shared__ uint32_t part[kSortLanes];
    if (rebuild_skipped(status, predicated)) return;
    const int t = (int)threadIdx.x, chunk = (total + kSortLanes - 1) / kSortLanes;
    const int first = t * chunk, end = first + chunk < total ? first + chunk : total;
    uint32_t sum = 0u;
    for (int j = first; j < end; j++) sum += hist[j];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < kSortLanes; off <<= 1)   // inclusive scan of the lanes' sums
    {
        const uint32_t add = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (int j = first; j < end; j++) { const uint32_t c = hist[j]; hist[j] = run; run += c; }
}

// stable: a key's place is its digit's base for this tile + the keys of the same digit before it in the tile
__global__ void __launch_bounds__(kRadixTile) k_radix_scatter(const uint32_t* codes, const uint32_t* idx, uint32_t* codes_out, uint32_t* idx_out, const uint32_t* hist,
                                                               const DeviceUpdateStatus* status, int n, int shift, int predicated)
{
    __shared__ uint32_t wave_cnt[kRadixTile / 64][kRadixBins];
    if (rebuild_skipped(status, predicated)) return;
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int w = 0; w < kRadixTile / 64; w++) wave_cnt[w][t] = 0u;
    __syncthreads();
    const int  i = (int)(blockIdx.x * kRadixTile + t);
    const bool live = i < n;
    const uint32_t code = live ? codes[i] : 0u, payload = live ? idx[i] : 0u;
    const uint32_t d = (code >> shift) & (kRadixBins - 1);
    unsigned long long peers = __ballot(live);   // the lanes of this wave that hold the same digit
    for (int b = 0; b < kRadixBits; b++)
    {
        const bool bit = (d >> b) & 1u;
        const unsigned long long has = __ballot(bit);
        peers &= bit ? has : ~has;
    }
    const uint32_t before = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (live && before == 0u) wave_cnt[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (!live) return;
    uint32_t at = hist[(size_t)d * gridDim.x + blockIdx.x] + before;
    for (int w = 0; w < wave; w++) at += wave_cnt[w][d];
    if (at < (uint32_t)n) { codes_out[at] = code; idx_out[at] = payload; }   // always true while hist is this pass's; the guard keeps a stale one in bounds
}

// bytes of the histogram radix_sort_enqueue needs for n keys
inline size_t radix_hist_bytes(size_t n) { return (size_t)kRadixBins * ((n + kRadixTile - 1) / kRadixTile) * 4; }

// codes[0] / idx[0] hold the n codes and ascending indices; an even number of passes: the order ends in idx[0].  Adds its launches to *launched.
inline hr_status radix_sort_enqueue(uint32_t* const codes[2], uint32_t* const idx[2], uint32_t* hist, const DeviceUpdateStatus* status, int n, int pred, hipStream_t st,
                                    int64_t* launched)
{
    const int blocks = cdiv(n, kRadixTile);
    for (int p = 0; p < kRadixPasses; p++)
    {
        const int in = p & 1, out = in ^ 1, shift = p * kRadixBits;
        hipLaunchKernelGGL(k_radix_hist, dim3(blocks), dim3(kRadixTile), 0, st, (const uint32_t*)codes[in], hist, status, n, shift, pred);
        HR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_radix_scan, dim3(1), dim3(kSortLanes), 0, st, hist, status, kRadixBins * blocks, pred);
        HR_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_radix_scatter, dim3(blocks), dim3(kRadixTile), 0, st, (const uint32_t*)codes[in], (const uint32_t*)idx[in], codes[out], idx[out],
                           (const uint32_t*)hist, status, n, shift, pred);
        HR_HIP(hipGetLastError());
        *launched += 3;
    }
    return HR_OK;
}

} // namespace
} // namespace hr
