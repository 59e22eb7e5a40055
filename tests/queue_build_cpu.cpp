// queue_build_cpu.cpp -- a stand-alone run of csrc/flx_queue_build.h, built by tests/test_queue_build.py with g++ -fsanitize=address,undefined and
// never loaded into Python.  It walks the membership bytes the way logic.hip does -- k_logic's tail (block counts, segment totals, counter
// snapshot), then k_queue_build block by block, wave by wave, lane by lane -- with every index computed by the header's functions, over heap
// buffers of exactly the sizes the lists need, so that a slot or a membership byte out of range is a sanitizer report.
//
//   queue_build_cpu <in> <out>
//   in : u32 numTasks, numCUs, perCU, snapshot[7]; numTasks membership bytes
//   out: u32 grid, parts, counters[7]; then for the 7 lists, the material union and the traced union: u32 n, n x u32 queue entries
//        (a list's queue is snapshot + count entries long and pre-filled with 0xFFFFFFFF; the unions start at slot 0)
#include "../fluctus_amd/csrc/flx_queue_build.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace flxqb;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: queue_build_cpu <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t head[3 + QB_LISTS];
    if (fread(head, 4, 3 + QB_LISTS, f) != 3 + QB_LISTS) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t numTasks = head[0], numCUs = head[1], perCU = head[2];
    const uint32_t *snapshot = head + 3;
    std::vector<uint8_t> member(numTasks);
    if (numTasks && fread(member.data(), 1, numTasks, f) != numTasks) { fprintf(stderr, "short member bytes\n"); return 2; }
    fclose(f);

    // ---- k_logic's tail: per block and list a count, added to the segment's total
    const uint32_t nb = qb_blocks(numTasks), nseg = qb_segments(numTasks), stride = qb_count_stride(numTasks);
    std::vector<uint32_t> counts((size_t)QB_LISTS * stride, 0u), totals(qb_totals_words(numTasks), 0u);
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < QB_LISTS; l++) {
            uint32_t s = 0;
            for (uint32_t t = 0; t < QB_BLOCK; t++) { const uint64_t p = (uint64_t)b * QB_BLOCK + t; if (p < numTasks) s += qb_in_list(member[p], l); }
            counts[(size_t)l * stride + b] = s;
            totals[(size_t)l * nseg + b / QB_SEG_BLOCKS] += s;
        }

    // ---- the lists' sizes (for buffers of exactly that size)
    uint32_t n[QB_LISTS + 2] = {0};
    for (uint32_t p = 0; p < numTasks; p++) {
        bool mat = false;
        for (uint32_t l = 0; l < QB_LISTS; l++) if (qb_in_list(member[p], l)) { n[l]++; if (l >= 2u) mat = true; }
        if (mat) n[QB_LISTS]++;
        if (mat || (member[p] & 1u)) n[QB_LISTS + 1]++;
    }
    std::vector<std::vector<uint32_t>> q(QB_LISTS + 2);
    for (uint32_t l = 0; l < QB_LISTS + 2; l++) q[l].assign((size_t)(l < QB_LISTS ? snapshot[l] : 0u) + n[l], 0xFFFFFFFFu);

    // ---- k_queue_build
    const uint32_t grid = qb_grid(nseg, numCUs, perCU), parts = qb_parts(nseg, numCUs, perCU);
    uint32_t counters[QB_LISTS] = {0};
    for (uint32_t block = 0; block < grid; block++) {
        uint32_t seg0, seg1;
        qb_owned(block, grid, nseg, parts, &seg0, &seg1);
        uint32_t tile0, steps;
        qb_tiles(block, parts, &tile0, &steps);
        if (seg0 > seg1 || seg1 > nseg) { fprintf(stderr, "block %u owns [%u, %u) of %u\n", block, seg0, seg1, nseg); return 1; }
        uint32_t base[QB_LISTS], fresh[QB_LISTS];
        for (uint32_t l = 0; l < QB_LISTS; l++) {
            uint32_t before = 0, all = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {          // the wave's partial sums, then its reduction
                uint32_t b, a;
                qb_partial(totals.data() + (size_t)l * nseg, nseg, seg0, lane, 64u, &b, &a);
                before += b; all += a;
            }
            base[l] = snapshot[l] + before; fresh[l] = snapshot[l] + all;
        }
        if (block == 0u) for (uint32_t l = 0; l < QB_LISTS; l++) counters[l] = fresh[l];
        for (uint32_t seg = seg0; seg < seg1; seg++) {
            std::vector<uint32_t> off((size_t)QB_LISTS * QB_SEG_BLOCKS);
            for (uint32_t l = 0; l < QB_LISTS; l++)
                for (uint32_t j = 0; j < QB_SEG_BLOCKS; j++) { off[l * QB_SEG_BLOCKS + j] = base[l]; base[l] += counts[(size_t)l * stride + (size_t)seg * QB_SEG_BLOCKS + j]; }
            for (uint32_t wave = 0; wave < QB_WAVES; wave++)
                for (uint32_t i = 0; i < steps; i++) {
                    const uint32_t tile = tile0 + wave + QB_WAVES * i;
                    uint32_t run[QB_LISTS + 2] = {0};             // the lanes below: what the ballots count
                    uint32_t matOff = 0;
                    for (uint32_t l = 2; l < QB_LISTS; l++) matOff += off[l * QB_SEG_BLOCKS + tile];
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        const uint64_t p = qb_first_path(seg, tile, lane);
                        const uint32_t valid = qb_valid(p, numTasks);
                        uint32_t w = 0;
                        for (uint32_t k = 0; k < valid; k++) w |= (uint32_t)member.at(p + k) << (8u * k);
                        for (uint32_t l = 0; l < QB_LISTS + 2; l++) {
                            const uint32_t bits = l < QB_LISTS ? qb_bits(w, l) : l == QB_LISTS ? qb_bits_material(w) : qb_bits_traced(w);
                            const uint32_t tileOff = l < QB_LISTS ? off[l * QB_SEG_BLOCKS + tile]
                                                   : l == QB_LISTS ? matOff - (snapshot[2] + snapshot[3] + snapshot[4] + snapshot[5] + snapshot[6])
                                                   : matOff + off[tile] - (snapshot[0] + snapshot[2] + snapshot[3] + snapshot[4] + snapshot[5] + snapshot[6]);
                            for (uint32_t k = 0; k < 4; k++)
                                if (bits & (1u << k)) {
                                    const size_t slot = (size_t)tileOff + run[l] + qb_rank4(bits, k);
                                    if (slot >= q[l].size()) { fprintf(stderr, "list %u: slot %zu of %zu\n", l, slot, q[l].size()); return 1; }
                                    if (q[l][slot] != 0xFFFFFFFFu) { fprintf(stderr, "list %u: slot %zu written twice\n", l, slot); return 1; }
                                    q[l][slot] = (uint32_t)p + k;
                                }
                            run[l] += qb_count4(bits);
                        }
                    }
                }
        }
    }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(&grid, 4, 1, f);
    fwrite(&parts, 4, 1, f);
    fwrite(counters, 4, QB_LISTS, f);
    for (uint32_t l = 0; l < QB_LISTS + 2; l++) {
        const uint32_t len = (uint32_t)q[l].size();
        fwrite(&len, 4, 1, f);
        if (len) fwrite(q[l].data(), 4, len, f);
    }
    fclose(f);
    printf("ok\n");
    return 0;
}
