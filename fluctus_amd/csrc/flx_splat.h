// flx_splat.h -- wave-cooperative accumulation into float4 records: one memory-side request per record instead of one per component.
//
// A float atomic executes at the memory side, and what it costs there is the REQUEST, not the bytes: a lane that adds the four words of its
// pixel {r, g, b, n} with four atomic instructions sends four requests of 4 useful bytes each, and a wave-instruction of ~13 terminating
// lanes touches ~13 different 64-byte pieces.  Here four adjacent lanes carry the four components of one predicated lane's record, so a
// record is ONE contiguous, aligned 16-byte piece of one instruction and an instruction serves up to 16 records.
// scripts/ubench/splat_shapes.hip (profiles/splat_shapes.txt): 1.76 M records of 8.4 M lanes into a 33 MB framebuffer, nothing else running,
// 0.349 ms as four instructions per lane and 0.086 ms transposed -- the memory path does merge the four lanes of a 16-byte group; behind the
// fused logic pass's streaming pattern most of that hides (0.505 -> 0.489 ms on one box, inside the spread on another; the product's figures:
// DESIGN.md 4.8, profiles/splat_ab.txt).  Cross-lane moves, a wave-private LDS stage and a block-wide LDS compaction measure the same within
// their spread; the cross-lane form needs no LDS and no barrier, so that is the one here.
#pragma once
#include "flx_device.h"

namespace flxd {

// base[4 * index + k] += {a, b, c, d}[k] for every lane with `pred`, k over the bits set in compMask (wave-uniform; a component whose bit is
// clear is not touched: no add of 0.0f).  Call it where the wave is convergent, lanes with `pred` false included.  Lanes that are not active
// at the call site are never read: ballots and permutes only see active lanes, and a wave that is not complete at the call site (the tail of
// the last wave, a launch bounded by the pixel count) takes the plain route, every predicated lane adding its own words.  More than 16
// predicated lanes take further rounds; lanes of one round that name the same index are separate lanes of one atomic instruction, and the
// memory side adds them all, as it does for two lanes of today's instruction.  No LDS, no global memory besides the adds, no waiting.
__device__ __forceinline__ void wave_add4(float *base, bool pred, uint32_t index, float a, float b, float c, float d, uint32_t compMask)
{
    const uint64_t active = __ballot(true);
    if (active != ~0ull) {
        if (pred) {
            float *px = base + (size_t)index * 4;
            if (compMask & 1u) unsafeAtomicAdd(px + 0, a);
            if (compMask & 2u) unsafeAtomicAdd(px + 1, b);
            if (compMask & 4u) unsafeAtomicAdd(px + 2, c);
            if (compMask & 8u) unsafeAtomicAdd(px + 3, d);
        }
        return;
    }
    const uint64_t tb = __ballot(pred);
    if (tb == 0ull) return;
    const uint32_t n = (uint32_t)__popcll(tb), lane = lane_id(), rank = mbcnt(tb);
    // a permutation of the 64 lanes: the predicated lanes first, in lane order, then the others -- every lane receives exactly one value
    const int dest = (int)((pred ? rank : n + lane - rank) << 2);
    const int ci = __builtin_amdgcn_ds_permute(dest, (int)index);
    const int c0 = __builtin_amdgcn_ds_permute(dest, __float_as_int(a)), c1 = __builtin_amdgcn_ds_permute(dest, __float_as_int(b));
    const int c2 = __builtin_amdgcn_ds_permute(dest, __float_as_int(c)), c3 = __builtin_amdgcn_ds_permute(dest, __float_as_int(d));
    const uint32_t comp = lane & 3u;
    const bool keep = ((compMask >> comp) & 1u) != 0u;
    for (uint32_t first = 0u; first < n; first += 16u) {                  // lane 4k + comp adds component comp of the (first + k)-th predicated lane
        const uint32_t s = first + (lane >> 2);                           // (< 64 whenever s < n)
        const int src = (int)((s & 63u) << 2);
        const int pi = __builtin_amdgcn_ds_bpermute(src, ci);
        const int w0 = __builtin_amdgcn_ds_bpermute(src, c0), w1 = __builtin_amdgcn_ds_bpermute(src, c1);
        const int w2 = __builtin_amdgcn_ds_bpermute(src, c2), w3 = __builtin_amdgcn_ds_bpermute(src, c3);
        const int w = comp == 0u ? w0 : comp == 1u ? w1 : comp == 2u ? w2 : w3;
        if (s < n && keep) unsafeAtomicAdd(base + (size_t)(uint32_t)pi * 4 + comp, __int_as_float(w));
    }
}

}  // namespace flxd
