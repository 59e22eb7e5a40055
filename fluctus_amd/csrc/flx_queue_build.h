// flx_queue_build.h -- the index arithmetic of the queue build (logic.hip: k_queue_build): which persistent block owns which paths, where its
// part of a list begins, and where a path lands inside a tile.  Plain C++ that compiles for the host and the device, so the CPU test
// (tests/queue_build_cpu.cpp) runs the very functions the kernel runs.
//
// THE SCHEME.  k_logic leaves one membership byte per path (bit0 raygen, bit1 shadow, bits 2..4 material list 0..5), seven counts per 256-path
// BLOCK, and -- with one fire-and-forget integer add per list and block -- seven totals per SEGMENT of QB_SEG_BLOCKS consecutive blocks; block 0
// also copies the seven queue counters as they stand before the pass (the SNAPSHOT: the lists append behind what the queues hold).  The build
// kernel is ONE launch of a grid sized by the machine.  Persistent block b owns the segments [b * share, (b + 1) * share), share =
// ceil(segments / grid), clipped to the segment count (the last blocks may own nothing).  It
//   1. sums, per list, the totals of ALL segments and of the segments in front of its own: base = snapshot + the latter, the new counter =
//      snapshot + the former (block 0 stores it).  At most ~1000 words per list, resident in L2; a block-wide reduction, no other block involved;
//   2. per owned segment turns the QB_SEG_BLOCKS block counts of each list into running offsets (one wave scan per list);
//   3. streams the segment's membership bytes as TILES of QB_TILE = 256 paths, one tile per wave and step, four bytes per lane: the lane's
//      paths of a list are ranked by the lanes below it (three ballots: the bits of the lane's count 0..4) plus its own earlier bytes.
// Nothing waits for another block: every dependency goes through the kernel boundary.  The result is the STABLE compaction by path id the
// scan + scatter pair produced: slot(path) = snapshot + #{paths with a smaller id in the list}.
//
// THE TOTALS ARE ZEROED WITHOUT A LAUNCH: two buffers, chosen by the parity of the pass; the build kernel of pass k zeroes the buffer that pass
// k + 1 adds into (pass k - 1's: its last reader was build k - 1, which is complete).  Both start zero-filled.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLX_QB_HD __host__ __device__ inline
#else
#define FLX_QB_HD inline
#endif

namespace flxqb {

enum : uint32_t {
    QB_LISTS = 7u,          // raygen, shadow, five material lists
    QB_BLOCK = 256u,        // paths per k_logic block = per block count
    QB_SEG_BLOCKS = 64u,    // blocks per segment: one lane of a wave per block count
    QB_SEG_PATHS = QB_BLOCK * QB_SEG_BLOCKS,
    QB_TILE = 256u,         // paths a wave ranks per step: 64 lanes x 4 membership bytes (== QB_BLOCK: a tile's offsets are a block's)
    QB_THREADS = 256u,      // threads of a build block: 4 waves
    QB_WAVES = QB_THREADS / 64u,
    QB_STEPS = QB_SEG_BLOCKS / QB_WAVES,    // tiles per wave and segment
    QB_MAX_PARTS = QB_STEPS                 // blocks that may share a segment (small wavefronts): each wave keeps one tile at least
};

FLX_QB_HD uint32_t qb_blocks(uint32_t numTasks) { return (uint32_t)(((uint64_t)numTasks + QB_BLOCK - 1u) / QB_BLOCK); }
FLX_QB_HD uint32_t qb_segments(uint32_t numTasks) { return (qb_blocks(numTasks) + QB_SEG_BLOCKS - 1u) / QB_SEG_BLOCKS; }
// words between two lists of the block counts: whole segments (the counts behind the last block stay zero)
FLX_QB_HD uint32_t qb_count_stride(uint32_t numTasks) { const uint32_t s = qb_segments(numTasks); return (s ? s : 1u) * QB_SEG_BLOCKS; }
// words of ONE totals buffer (there are two, then the snapshot)
FLX_QB_HD uint32_t qb_totals_words(uint32_t numTasks) { const uint32_t s = qb_segments(numTasks); return QB_LISTS * (s ? s : 1u); }
FLX_QB_HD uint32_t qb_aux_words(uint32_t numTasks) { return 2u * qb_totals_words(numTasks) + 8u; }
FLX_QB_HD uint32_t qb_snapshot_at(uint32_t numTasks) { return 2u * qb_totals_words(numTasks); }

// persistent grid: `perCU` blocks per compute unit, at least one block (it stores the counters).  A wavefront with fewer segments than that
// (1 M paths are 64) would leave most of the machine idle, so there a segment is split into `parts` runs of tiles, one block each: the largest
// power of two <= QB_MAX_PARTS (a wave per tile at least) that still fits the cap.  With parts > 1 a block owns exactly one part of one segment.
FLX_QB_HD uint64_t qb_cap(uint32_t numCUs, uint32_t perCU) { return (uint64_t)(numCUs ? numCUs : 1u) * (perCU ? perCU : 1u); }
FLX_QB_HD uint32_t qb_parts(uint32_t segments, uint32_t numCUs, uint32_t perCU)
{
    uint32_t parts = 1u;
    while (parts < QB_MAX_PARTS && (uint64_t)segments * (2u * parts) <= qb_cap(numCUs, perCU)) parts *= 2u;
    return parts;
}
FLX_QB_HD uint32_t qb_grid(uint32_t segments, uint32_t numCUs, uint32_t perCU)
{
    const uint64_t cap = qb_cap(numCUs, perCU), units = (uint64_t)segments * qb_parts(segments, numCUs, perCU);
    const uint32_t g = units < cap ? (uint32_t)units : (uint32_t)cap;
    return g ? g : 1u;
}
FLX_QB_HD uint32_t qb_share(uint32_t segments, uint32_t grid) { return (segments + grid - 1u) / grid; }
FLX_QB_HD void qb_owned(uint32_t block, uint32_t grid, uint32_t segments, uint32_t parts, uint32_t *first, uint32_t *end)
{
    const uint64_t share = parts > 1u ? 1u : qb_share(segments, grid);
    const uint64_t f = parts > 1u ? block / parts : share * block, e = f + share;
    *first = f < segments ? (uint32_t)f : segments;
    *end = e < segments ? (uint32_t)e : segments;
}
// the tiles of an owned segment that are the block's: tile0 + wave + QB_WAVES * i for i < steps
FLX_QB_HD void qb_tiles(uint32_t block, uint32_t parts, uint32_t *tile0, uint32_t *steps)
{
    *tile0 = (block % parts) * (QB_SEG_BLOCKS / parts);
    *steps = QB_STEPS / parts;
}

// thread t of n: its part of one list's sums over the segment totals -- all of them, and those in front of segment `first`
FLX_QB_HD void qb_partial(const uint32_t *totals, uint32_t segments, uint32_t first, uint32_t t, uint32_t n, uint32_t *before, uint32_t *all)
{
    uint32_t b = 0u, a = 0u;
    for (uint32_t s = t; s < segments; s += n) { const uint32_t v = totals[s]; a += v; if (s < first) b += v; }
    *before = b; *all = a;
}

// four membership bytes (little endian: byte k = path 4 * lane + k of the tile) -> bit k set = path k is in the list
FLX_QB_HD uint32_t qb_in_list(uint32_t byte, uint32_t list)      // list 0 raygen, 1 shadow, 2..6 material list 1..5
{
    return list == 0u ? (byte & 1u) : list == 1u ? ((byte >> 1) & 1u) : (((byte >> 2) & 7u) == list - 1u ? 1u : 0u);
}
FLX_QB_HD uint32_t qb_bits(uint32_t word, uint32_t list)
{
    return qb_in_list(word & 0xFFu, list) | (qb_in_list((word >> 8) & 0xFFu, list) << 1) | (qb_in_list((word >> 16) & 0xFFu, list) << 2) | (qb_in_list(word >> 24, list) << 3);
}
// ... = path k has a material list at all (the continuing paths), and: that or the raygen bit (every path that will be traced)
FLX_QB_HD uint32_t qb_bits_material(uint32_t word)
{
    const uint32_t m = word & 0x1C1C1C1Cu;                        // bits 2..4 of every byte
    const uint32_t any = (m | (m >> 1) | (m >> 2)) & 0x04040404u;   // bit 2 of byte k = one of them set
    return ((any >> 2) | (any >> 9) | (any >> 16) | (any >> 23)) & 0xFu;
}
FLX_QB_HD uint32_t qb_bits_traced(uint32_t word)
{
    const uint32_t r = word & 0x01010101u;
    return (qb_bits_material(word) | r | (r >> 7) | (r >> 14) | (r >> 21)) & 0xFu;
}
FLX_QB_HD uint32_t qb_count4(uint32_t bits) { return (bits & 1u) + ((bits >> 1) & 1u) + ((bits >> 2) & 1u) + ((bits >> 3) & 1u); }
// a lane's path k: its rank among the lane's own paths of the list
FLX_QB_HD uint32_t qb_rank4(uint32_t bits, uint32_t k) { return qb_count4(bits & ((1u << k) - 1u)); }
// first path of lane `lane`'s four bytes in tile `tile` (= block) of segment `seg`: 64 bits, a grid of whole segments may reach past 2^32
FLX_QB_HD uint64_t qb_first_path(uint32_t seg, uint32_t tile, uint32_t lane) { return ((uint64_t)seg * QB_SEG_BLOCKS + tile) * QB_TILE + 4u * lane; }
// the bytes at or behind numTasks do not exist: how many of the four bytes from path p on may be read
FLX_QB_HD uint32_t qb_valid(uint64_t p, uint32_t numTasks) { return p >= numTasks ? 0u : numTasks - p >= 4u ? 4u : (uint32_t)(numTasks - p); }

}  // namespace flxqb
