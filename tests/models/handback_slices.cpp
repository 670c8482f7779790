// handback_slices.cpp — host check of the slice rule of the co-scheduled hand-back list (zoe_amd/csrc/zsw_handback.hpp:
// handback_slice_rule, handback_slices — the text launch_score_seeded and handback_split_kernel compile). The frozen list
// [0, n0) is scored by up to three launches: the first tier's shared launch, a head slice and a tail slice on side streams. Each
// reads its range from device words (ScoreArgsV2::first_item_dev / n_items_dev) and its grid is sized on the host; a read no
// launch takes keeps the caller's fill, a read two launches take is scored twice.
//
// usage: handback_slices sweep     every rule the switches and the host-known facts can give, every n0 in 0 .. 3 x (head + tail + one
//            round): the three ranges are disjoint, in order and cover [0, n0); by score_body_v2's own index arithmetic every read
//            is taken by exactly one launch; no slice is longer than its grid; a slice is all or nothing (but the tiny head); the
//            shared part keeps a round wherever a slice is cut; the thresholds sit where the header says. One line per violation,
//            then "handback_slices sweep: <checks> checks, <v> violations".
//        handback_slices decide    one line "DECIDE <coschedule bits> own no_slices tiny class -> head tail" per case
//        handback_slices budget    "BUDGET tail_waves tail_vgprs band_vgprs remainder_vgprs per_simd tail_reads tail_G"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zoe_amd/csrc/zsw_handback.hpp"

using namespace zsw;

static_assert(handback_slices(0, handback_slice_rule(true, true, 10000000, false, false)).tail.end == 0, "the rule is usable in constant expressions");
static_assert(HANDBACK_TAIL_READS <= HANDBACK_TAIL_WAVES_PER_SIMD * HANDBACK_SIMDS * (128 / HANDBACK_TAIL_G), "a wavefront of G lanes per pair holds 128 / G reads");

namespace {

long checks = 0, violations = 0;

// the reads [first, end) a launch of score_kernel_v2 takes (zsw_score_v2.hpp: score_body_v2): n_list = *n_items_dev, first =
// min(*first_item_dev, n_list), n_items = min(n_list - first, b.n_items); a block returns unless 2 * block * (BLOCK / G) < n_items,
// and the grid has handback_blocks(b.n_items, G) blocks
ItemRange launch_takes(uint32_t first_word, uint32_t end_word, uint32_t grid_items, int G) {
    const uint32_t n_list = end_word, first = std::min(first_word, n_list), n_items = std::min(n_list - first, grid_items);
    const uint64_t grid_reads = (uint64_t)handback_blocks(grid_items, G) * 2 * handback_block_pairs(G);
    return ItemRange{first, first + (uint32_t)std::min<uint64_t>(n_items, grid_reads)};
}

void violation(const char* what, const HandbackSliceRule& r, uint32_t n0, const HandbackSlices& s) {
    std::printf("VIOLATION %s: rule keep %u tail %u/%u head %u/%u, n0 %u -> shared [%u, %u) head [%u, %u) tail [%u, %u)\n", what, r.keep, r.tail_reads, r.tail_min,
                r.head_reads, r.head_min, n0, s.shared.first, s.shared.end, s.head.first, s.head.end, s.tail.first, s.tail.end);
    ++violations;
}

void check_rule(const HandbackSliceRule& r, uint32_t class_reads, uint32_t n0_max, bool exact_sizes) {
    std::vector<uint8_t> taken;
    for (uint32_t n0 = 0; n0 <= n0_max; ++n0) {
        ++checks;
        const HandbackSlices s = handback_slices(n0, r);
        const uint32_t head = s.head.end - s.head.first, tail = s.tail.end - s.tail.first;
        if (s.shared.first != 0 || s.shared.end != s.head.first || s.head.end != s.tail.first || s.tail.end != n0 || s.shared.end > s.head.end || s.head.end > n0)
            violation("the ranges do not partition [0, n0)", r, n0, s);
        if (head > r.head_reads || tail > r.tail_reads) violation("a slice beyond its bound", r, n0, s);
        if ((head && head < r.head_min) || (tail && tail < r.tail_min)) violation("a slice below its minimum", r, n0, s);
        if (exact_sizes && ((head && head != r.head_reads) || (tail && tail != r.tail_reads))) violation("a partial slice", r, n0, s);
        if ((head || tail) && s.shared.end < r.keep) violation("the shared launch keeps less than a round", r, n0, s);
        // the thresholds: the tail is cut from keep + tail_min on, the head from keep + tail + head_min on
        const bool want_tail = r.tail_reads && n0 >= r.keep + r.tail_min;
        const bool want_head = r.head_reads && n0 >= r.keep + (want_tail ? std::min(n0 - r.keep, r.tail_reads) : 0u) + r.head_min;
        if (want_tail != (tail != 0) || want_head != (head != 0)) violation("a threshold is not where the header says", r, n0, s);
        // the launches: the shared one over [0, bounds[0]) with the class's grid, the slices with grids of their bounds
        const ItemRange got[3] = {launch_takes(0, s.shared.end, class_reads, 4), r.head() ? launch_takes(s.head.first, s.head.end, r.head_reads, 4) : ItemRange{0, 0},
                                  r.tail() ? launch_takes(s.tail.first, s.tail.end, r.tail_reads, HANDBACK_TAIL_G) : ItemRange{0, 0}};
        uint64_t sum = 0;
        for (const ItemRange& g : got) sum += g.end - g.first;
        const bool in_order = got[0].first == 0 && got[0].end == s.shared.end && (got[1].first == got[1].end || (got[1].first == s.head.first && got[1].end == s.head.end)) &&
                              (got[2].first == got[2].end || (got[2].first == s.tail.first && got[2].end == s.tail.end));
        if (sum != n0 || !in_order) violation("not every read is taken by exactly one launch", r, n0, s);
        if (n0 <= 1024) {  // ... and read by read
            taken.assign(n0, 0);
            for (const ItemRange& g : got)
                for (uint32_t i = g.first; i < g.end && i < n0; ++i) ++taken[i];
            if (std::count(taken.begin(), taken.end(), 1) != (long)n0) violation("a read taken twice or not at all", r, n0, s);
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "budget") == 0) {
        std::printf("BUDGET %u %u %u %u %u %u %d\n", HANDBACK_TAIL_WAVES_PER_SIMD, HANDBACK_VGPRS_TAIL, HANDBACK_VGPRS_BAND, HANDBACK_VGPRS_REMAINDER, HANDBACK_VGPRS_PER_SIMD,
                    HANDBACK_TAIL_READS, HANDBACK_TAIL_G);
        return 0;
    }
    const uint32_t classes[] = {0u, 1u, 4097u, HANDBACK_SLICE_MIN_CLASS - 1, HANDBACK_SLICE_MIN_CLASS, 10000000u};
    if (argc == 2 && std::strcmp(argv[1], "decide") == 0) {
        const int gs[] = {4, 8};
        for (int mode = 0; mode < 3; ++mode)
            for (int g : gs)
                for (int bits = 0; bits < 512; ++bits)
                    for (uint32_t cls : classes) {
                        CoscheduleCase c{};
                        c.mode = mode;
                        c.G = g;
                        c.two_tiers = bits & 1;
                        c.diagonal = bits & 2;
                        c.mins = bits & 4;
                        c.row_chunks = bits & 8;
                        c.skip_handed_back = bits & 16;
                        c.disabled = bits & 32;
                        const bool own = bits & 64, no_slices = bits & 128, tiny = bits & 256;
                        const HandbackSliceRule r = handback_slice_rule(handback_coschedule(c), own, cls, no_slices, tiny);
                        std::printf("DECIDE %d %d %d %d %d %d %d %d %d %d %d %d %u -> %u %u\n", mode, (int)c.two_tiers, (int)c.diagonal, g, (int)c.mins, (int)c.row_chunks,
                                    (int)c.skip_handed_back, (int)c.disabled, (int)handback_coschedule(c), (int)own, (int)no_slices, (int)tiny, cls, r.head_reads, r.tail_reads);
                    }
        return 0;
    }
    if (argc != 2 || std::strcmp(argv[1], "sweep") != 0) return 2;
    const uint32_t n0_max = 3 * (HANDBACK_HEAD_READS + HANDBACK_TAIL_READS + HANDBACK_ROUND_READS);
    for (uint32_t cls : classes)
        for (int sw = 0; sw < 8; ++sw) {
            const bool own = sw & 1, no_slices = sw & 2, tiny = sw & 4;
            const HandbackSliceRule r = handback_slice_rule(true, own, cls, no_slices, tiny);
            // (the count on the device is at most the class; the rule must hold for any count all the same)
            check_rule(r, std::max(cls, n0_max), n0_max, !tiny);
        }
    // the rule's own edges, whatever the constants: a head or a tail alone, minimums below the sizes
    const HandbackSliceRule edges[] = {{0, 0, 0, 128, 128}, {0, 128, 128, 0, 0}, {256, 0, 0, 128, 1}, {256, 128, 1, 0, 0}, {1, 3, 2, 5, 4}, {384, 128, 128, 128, 128}};
    for (const HandbackSliceRule& r : edges) check_rule(r, 4096, 3 * (r.keep + r.head_reads + r.tail_reads) + 8, false);
    std::printf("handback_slices sweep: %ld checks, %ld violations\n", checks, violations);
    return 0;
}
