// coschedule_plan.cpp — host check of the co-scheduled full pass's plain-C++ side (zoe_amd/csrc/zsw_handback.hpp, the text
// launch_score_seeded and seed_diag_handback_kernel compile): which calls score the seed kernel's hand-backs inside the first band
// tier's launch, and how that launch's grid is split.
//
// usage: coschedule_plan split <n_items> <count> ...   for every G in {4, 8, 16, 32, 64} and a band grid of 1, 7 and 1,024 blocks:
//            every block of the grid has one role; the hand-back indexes are 0 .. hb_blocks - 1 in order, the band indexes
//            0 .. grid - 1; every pair of a list of `count` reads is owned by exactly one hand-back block, in order, and no block
//            owns a pair beyond the list. Prints one line per violation, then "coschedule_plan split: <checks> checks, <v> violations".
//        coschedule_plan decide                      one line "DECIDE mode two_tiers diagonal G mins row_chunks skip disabled -> 0|1" per case
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zoe_amd/csrc/zsw_handback.hpp"

using namespace zsw;

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "decide") == 0) {
        const int gs[] = {4, 8, 16, 32, 64};
        for (int mode = 0; mode < 4; ++mode)
            for (int g : gs)
                for (int bits = 0; bits < 64; ++bits) {
                    CoscheduleCase c{};
                    c.mode = mode;
                    c.G = g;
                    c.two_tiers = bits & 1;
                    c.diagonal = bits & 2;
                    c.mins = bits & 4;
                    c.row_chunks = bits & 8;
                    c.skip_handed_back = bits & 16;
                    c.disabled = bits & 32;
                    std::printf("DECIDE %d %d %d %d %d %d %d %d -> %d\n", mode, (int)c.two_tiers, (int)c.diagonal, g, (int)c.mins, (int)c.row_chunks,
                                (int)c.skip_handed_back, (int)c.disabled, (int)handback_coschedule(c));
                }
        return 0;
    }
    if (argc < 4 || std::strcmp(argv[1], "split") != 0 || (argc - 2) % 2 != 0) return 2;
    long checks = 0, violations = 0;
    const int gs[] = {4, 8, 16, 32, 64};
    const uint32_t grids[] = {1, 7, 1024};
    for (int i = 2; i + 1 < argc; i += 2) {
        const uint32_t n_items = (uint32_t)std::strtoul(argv[i], nullptr, 10), count = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10);
        if (count > n_items) return 2;
        for (int g : gs) {
            const uint32_t hb = handback_blocks(n_items, g);
            if ((uint64_t)hb * 2 * handback_block_pairs(g) < n_items || (hb && (uint64_t)(hb - 1) * 2 * handback_block_pairs(g) >= n_items)) {
                std::printf("VIOLATION n %u G %d: %u hand-back blocks\n", n_items, g, hb);
                ++violations;
            }
            for (uint32_t grid : grids) {  // the roles partition the grid
                ++checks;
                uint32_t next_hb = 0, next_band = 0;
                bool ok = true;
                for (uint32_t b = 0; b < hb + grid; ++b) {
                    const CoscheduleRole r = coschedule_role(b, hb);
                    ok = ok && r.index == (r.handback ? next_hb++ : next_band++) && (r.handback || next_hb == hb);
                }
                if (!ok || next_hb != hb || next_band != grid) {
                    std::printf("VIOLATION n %u G %d grid %u: roles %u + %u\n", n_items, g, grid, next_hb, next_band);
                    ++violations;
                }
            }
            // the pairs of the list, in order, each owned once
            ++checks;
            const uint32_t pairs = (uint32_t)(((uint64_t)count + 1) / 2);
            uint32_t next = 0;
            bool ok = true;
            for (uint32_t b = 0; b < hb; ++b) {
                const PairRange r = handback_block_range(b, g, count);
                // score_body_v2's own arithmetic (zsw_score_v2.hpp): the block returns if 2 * block * (BLOCK / G) >= count; thread tid
                // walks pair block * (BLOCK / G) + tid / G if its first read 2 * pair is below count
                uint32_t k_first = 0, k_end = 0;
                if ((uint64_t)2 * b * (HANDBACK_BLOCK_THREADS / g) < count) {
                    for (uint32_t tid = 0; tid < HANDBACK_BLOCK_THREADS; ++tid) {
                        const uint32_t pair = b * (HANDBACK_BLOCK_THREADS / g) + tid / g;
                        if ((uint64_t)2 * pair < count) {
                            if (k_first == k_end) k_first = pair;
                            k_end = pair + 1;
                        }
                    }
                }
                ok = ok && ((r.first == r.end && k_first == k_end) || (r.first == k_first && r.end == k_end));
                if (r.first == r.end) continue;
                ok = ok && r.first == next && r.end > r.first && r.end <= pairs && r.end - r.first <= handback_block_pairs(g);
                next = r.end;
            }
            if (!ok || next != pairs) {
                std::printf("VIOLATION n %u count %u G %d: pairs owned up to %u of %u\n", n_items, count, g, next, pairs);
                ++violations;
            }
        }
    }
    std::printf("coschedule_plan split: %ld checks, %ld violations\n", checks, violations);
    return 0;
}
