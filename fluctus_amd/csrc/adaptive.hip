// adaptive.hip -- flx_mk_adaptive_update: classify every pixel with the stopping rule of csrc/flx_adaptive.h and compact the
// active ones into an ASCENDING list for the list-driven microkernels (microkernel.hip: k_mk_*<true>).
//
// Three launches -- flag bytes and block counts, a one-block scan, a scatter; the pattern logic.hip's queues had before their scan and scatter became
// one persistent launch (k_queue_build; not worth it here: this runs once per adaptive update, not in every step) -- and no atomics at all:
//   k_ad_classify  one thread per pixel in 1-D blocks of 256 CONSECUTIVE pixels: the pixel's moments (16 B), the 3 x 3 neighbours' only where
//                  the pixel itself has converged (the rows above and below come out of L2), one flag byte, and the block's count of active
//                  pixels from four ballots.
//   k_ad_scan      one block: exclusive scan of the block counts, the total to the count word.
//   k_ad_scatter   flag byte -> ballot -> rank by mbcnt: list[block offset + waves before + rank] = pixel.  Blocks and lanes are in pixel
//                  order, so the list is ascending and equals tests/adaptive_cpu.cpp's exactly.
// Every flag comes from ad_pixel in its order, so it equals the counterpart's bit for bit.
#include "flx_device.h"
#include "flx_adaptive.h"
#include "flx_launch.h"

namespace flxd {

#define AD_BLOCK 256

__device__ __forceinline__ ad4 to_ad4(float4 v) { ad4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; return r; }

__global__ __launch_bounds__(AD_BLOCK) void k_ad_classify(const float4 *mom, int W, int H, ad_params ap, uint8_t *flags, uint32_t *blockCounts)
{
    __shared__ uint32_t s_cnt[AD_BLOCK / 64];
    const uint32_t npix = (uint32_t)W * (uint32_t)H;
    const uint32_t gid = blockIdx.x * AD_BLOCK + threadIdx.x;
    uint32_t f = 0u;
    if (gid < npix) {
        f = ad_pixel((int)(gid % (uint32_t)W), (int)(gid / (uint32_t)W), W, H, ap, [&](uint32_t j) { return to_ad4(mom[j]); });
        flags[gid] = (uint8_t)f;
    }
    const uint64_t b = __ballot((f & FLX_AD_ACTIVE) != 0u);
    if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) blockCounts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// one block: every thread owns a contiguous run of `per` block counts; the 16 waves scan their threads' sums with shuffles, wave 0 the 16
// wave totals. In place: blockCounts holds the exclusive offsets afterwards (every thread reads its own run before it
// overwrites it).
__global__ __launch_bounds__(1024) void k_ad_scan(uint32_t *blockCounts, uint32_t nb, uint32_t *count)
{
    __shared__ uint32_t s_wave[16];
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per;
    uint32_t s = 0;
    for (uint32_t i = 0; i < per; i++) if (lo + i < nb) s += blockCounts[lo + i];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = s;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    if (wave == 0u) {
        uint32_t w = lane < 16u ? s_wave[lane] : 0u, wi = w;
        for (int d = 1; d < 16; d <<= 1) { const uint32_t v = __shfl_up(wi, d, 64); if (lane >= (uint32_t)d) wi += v; }
        if (lane < 16u) s_wave[lane] = wi - w;
        if (lane == 15u) *count = wi;
    }
    __syncthreads();
    uint32_t run = s_wave[wave] + inc - s;
    for (uint32_t i = 0; i < per; i++)
        if (lo + i < nb) { const uint32_t v = blockCounts[lo + i]; blockCounts[lo + i] = run; run += v; }
}

__global__ __launch_bounds__(AD_BLOCK) void k_ad_scatter(const uint8_t *flags, uint32_t npix, const uint32_t *blockOffsets, uint32_t *list)
{
    __shared__ uint32_t s_cnt[AD_BLOCK / 64];
    const uint32_t gid = blockIdx.x * AD_BLOCK + threadIdx.x;
    const bool act = gid < npix && (flags[gid] & FLX_AD_ACTIVE) != 0u;
    const uint64_t b = __ballot(act);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_cnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (act) {
        uint32_t r = blockOffsets[blockIdx.x];
        for (uint32_t w = 0; w < wave; w++) r += s_cnt[w];
        list[r + mbcnt(b)] = gid;                   // r + rank < the total <= npix: the list holds npix entries
    }
}

uint32_t adaptive_blocks(uint32_t npix) { return (npix + AD_BLOCK - 1) / AD_BLOCK; }

// the scan on its own, for the other users of this scheme (pose.hip)
void launch_block_scan(hipStream_t s, uint32_t *blockCounts, uint32_t nb, uint32_t *total)
{
    hipLaunchKernelGGL(k_ad_scan, dim3(1), dim3(1024), 0, s, blockCounts, nb, total);
}

// mom: the moments of W x H pixels; flags: W * H bytes; blockScratch: adaptive_blocks(W * H) words; list: W * H words; count: one word
void launch_adaptive_update(hipStream_t s, const float4 *mom, int W, int H, const ad_params &ap, uint8_t *flags, uint32_t *blockScratch, uint32_t *list,
                            uint32_t *count)
{
    const uint32_t npix = (uint32_t)W * (uint32_t)H, nb = adaptive_blocks(npix);
    hipLaunchKernelGGL(k_ad_classify, dim3(nb), dim3(AD_BLOCK), 0, s, mom, W, H, ap, flags, blockScratch);
    launch_block_scan(s, blockScratch, nb, count);
    hipLaunchKernelGGL(k_ad_scatter, dim3(nb), dim3(AD_BLOCK), 0, s, flags, npix, blockScratch, list);
}

} // namespace flxd
