// zsw_handback.hpp — which launches of score_kernel_v2 score the reads the seeded pass hands back. Plain C++, no HIP: zsw_score.hip
// (seed_items) and the host model tests/models/handback_plan.cpp compile the same text.
//
// The length of the hand-back list stays on the device. A short list is latency-bound in the class's own strip configuration, a
// long one throughput-bound in any other, so the list is launched in up to three configurations — the ones the cost model picks for
// 16 k, 128 k and many reads — and each launch returns at once unless the count lies in its gate [lo, hi). Whatever the count is,
// EXACTLY ONE planned launch must take it: a count no gate holds leaves reads unscored and the caller's arrays as they were.
#pragma once
#include <algorithm>
#include <cstdint>

namespace zsw {

struct StripCfg {
    int G, C;  // lanes per read pair x columns per lane
};

// The first of the n_ascending configurations of ascending capacity G*C that holds max_len columns.
inline bool strip_config_first_fit(const StripCfg* cfgs, int n_ascending, uint32_t max_len, int* G, int* C) {
    for (int k = 0; k < n_ascending; ++k) {
        if ((uint32_t)(cfgs[k].G * cfgs[k].C) >= max_len) {
            *G = cfgs[k].G;
            *C = cfgs[k].C;
            return true;
        }
    }
    return false;
}

// Same, for a batch of n_items reads: a small batch cannot fill 1024 SIMDs with the narrowest strips (10 k reads of 150 bp are
// 312 wavefronts at G = 4), so it takes more lanes per read and fewer columns per lane. The score does not depend on the choice.
// Cost model: a step issues about 7.5*C + 25 instructions; a launch is latency-bound up to ~2 waves per SIMD, throughput-bound above.
inline bool strip_config_for_batch(const StripCfg* cfgs, int n_cfgs, uint32_t max_len, uint32_t n_items, int* G, int* C) {
    double best = 0;
    bool found = false;
    for (int k = 0; k < n_cfgs; ++k) {
        const StripCfg& c = cfgs[k];
        if ((uint32_t)(c.G * c.C) < max_len) continue;
        const double waves = ((double)((n_items + 1) / 2) * c.G) / 64.0;
        const double cost = (7.5 * c.C + 25.0) * std::max(2048.0, waves);
        if (!found || cost < best * 0.97) {  // ties go to the narrower configuration
            best = cost;
            *G = c.G;
            *C = c.C;
            found = true;
        }
    }
    return found;
}

constexpr uint32_t HANDBACK_CUTS[2] = {49152u, 327680u};    // a gate ends where the next begins
constexpr uint32_t HANDBACK_PROBE[2] = {16384u, 131072u};   // the list length whose configuration serves the range below each cut
constexpr int HANDBACK_MAX_LAUNCHES = 3;

struct HandbackLaunch {
    uint32_t lo, hi;      // the launch runs if lo <= count < hi
    int G, C;
    uint32_t grid_items;  // the grid is sized for this many reads (a longer list is not this launch's)
    bool own_tables;      // false: the class's configuration, with the tables its seeded pass was given
};

// The launches for a class of n_items reads of up to `longest` columns whose seeded pass ran in configuration (g, c).
// tables_ok(G): can the score tables of a configuration of G lanes be built? A range whose tables cannot is left to the next launch
// (lo stays), in the end to the class's own configuration. A range is planned whenever the count can reach it: n_items >= lo.
template <class TablesOk>
inline int handback_plan(const StripCfg* cfgs, int n_cfgs, uint32_t longest, int g, int c, uint32_t n_items, TablesOk tables_ok,
                         HandbackLaunch out[HANDBACK_MAX_LAUNCHES]) {
    int n = 0;
    uint32_t lo = 0;
    for (int k = 0; k < 3; ++k) {
        const uint32_t hi = k < 2 ? HANDBACK_CUTS[k] : 0xffffffffu;
        if (n_items == 0 || lo > n_items) break;  // (the count is at most n_items)
        int g2 = g, c2 = c;
        const bool other = k < 2 && strip_config_for_batch(cfgs, n_cfgs, longest, HANDBACK_PROBE[k], &g2, &c2) && g2 != g;
        if (k < 2 && (!other || !tables_ok(g2))) continue;  // (the class's configuration serves this range too: lo stays)
        out[n++] = other ? HandbackLaunch{lo, hi, g2, c2, std::min(n_items, hi), true} : HandbackLaunch{lo, hi, g, c, n_items, false};
        lo = hi;
    }
    return n;
}

// ---- the full pass co-scheduled with the first band tier (zsw_score_band.hip: seed_diag_handback_kernel) ----------------------------
// Nearly all of the hand-back list exists before the band tiers start: the seed kernel lists the reads without an anchor itself. In a
// two-tier call the first tier appends nothing (what it cannot prove is flagged for the second tier, and it never bails), so the list
// and its count are frozen while the first tier runs — and the full pass over that part of the list can share the first tier's grid:
// the first handback_blocks() blocks of the launch score list[0, count), the blocks behind them are the tier's persistent blocks.
// The gated launches of handback_plan then score list[count at that time, final count) only (ScoreArgsV2::first_item_dev).
// Host model: tests/models/coschedule_plan.cpp.
struct CoscheduleCase {
    int mode;               // 0 score only, 1 / 2 with ends
    bool two_tiers;         // a narrow first tier with `retry` flags and no bail-out, then the full band
    bool diagonal;          // ... walked diagonal by diagonal (seed_diag_kernel: it uses no blockIdx)
    int G;                  // lanes per read pair of the class's strip configuration
    bool mins;              // ZSW_OPTION_MIN_SCORE: the MINS instantiations
    bool row_chunks;        // the hand-backs are cut into chunks of rows (their results are folded by a kernel over the whole list)
    bool skip_handed_back;  // the caller settles the handed-back reads by other means
    bool disabled;          // ZSW_DEBUG_SEED_NO_COSCHEDULE
};
constexpr bool handback_coschedule(const CoscheduleCase& c) {
    return c.mode == 0 && c.two_tiers && c.diagonal && c.G == 4 && !c.mins && !c.row_chunks && !c.skip_handed_back && !c.disabled;
}

constexpr uint32_t HANDBACK_BLOCK_THREADS = 256;  // (= BLOCK of zsw_score_v2.hpp)
// pairs of reads per block of score_kernel_v2 in a configuration of G lanes per pair
constexpr uint32_t handback_block_pairs(int G) { return HANDBACK_BLOCK_THREADS / (uint32_t)G; }
// blocks of a grid sized for n_items reads (the count on the device is at most that)
constexpr uint32_t handback_blocks(uint32_t n_items, int G) { return (n_items + 2 * handback_block_pairs(G) - 1) / (2 * handback_block_pairs(G)); }
// A block of the co-scheduled grid: hand-back block `index` (its pairs below), or persistent block `index` of the band tier. The
// hand-back blocks take the low indices: blocks are dispatched in index order, so the long items start first (for speed only).
struct CoscheduleRole {
    bool handback;
    uint32_t index;
};
constexpr CoscheduleRole coschedule_role(uint32_t block, uint32_t hb_blocks) {
    return block < hb_blocks ? CoscheduleRole{true, block} : CoscheduleRole{false, block - hb_blocks};
}
// The pairs [first, end) of a list of `count` reads that hand-back block `block` scores (pair p = reads 2p and 2p + 1, the last pair of
// an odd count has no partner); first == end: the block returns at once.
struct PairRange {
    uint32_t first, end;
};
constexpr PairRange handback_block_range(uint32_t block, int G, uint32_t count) {
    const uint64_t pairs = ((uint64_t)count + 1) / 2, lo = (uint64_t)block * handback_block_pairs(G), hi = lo + handback_block_pairs(G);
    return lo >= pairs ? PairRange{0u, 0u} : PairRange{(uint32_t)lo, (uint32_t)(hi < pairs ? hi : pairs)};
}

}  // namespace zsw
