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

// ---- slices of the frozen list on side streams (zsw_score_seed.hip: launch_score_seeded; zsw_handback_split.hip) ---------------------
// The co-scheduled launch runs at the issue roof, and the kernels around it leave the vector units idle: the sort in front of it
// is memory-bound, the select / second tier / remainder behind it are a few thousand reads on an empty chip. The list is frozen
// from the seed kernel on, so a bounded slice of it can leave the shared grid and run as a plain launch of score_kernel_v2 on a
// side stream exactly there: `head` from behind the seed kernel (beside the sort), `tail` from behind the shared launch (beside
// the second tier). Measured, the head loses — beside it the sort's longest kernel takes 1.28 ms instead of 0.1 — so
// the default rule cuts no head (HANDBACK_HEAD_READS = 0); the tiny rule of the tests still does, and the code path is one.
// list[0, n0) = shared | head | tail, in that order; n0 is on the device, so a one-thread kernel behind the seed
// kernel evaluates handback_slices() there and the launches read their bounds from device words. Host model:
// tests/models/handback_slices.cpp.
//
// Sizes. A resident wavefront of the shared launch's score body holds 32 reads (<4, C>: 16 pairs), a round of it — three
// wavefronts on each of 1024 SIMDs — 98,304. A slice is all or nothing: a list that cannot give a whole slice AND leave the shared
// launch a full round keeps today's launches.
// The tail must not hold up the second tier: per SIMD its resident wavefronts share 512 VGPRs with one wavefront of
// seed_band_kernel<48,2,0> and one of the remainder launch score_kernel_v2<32,5,0>. From -Rpass-analysis=kernel-resource-usage
// (allocated in steps of 8): score_kernel_v2<4,38,0> 141 -> 144 (the widest four-lane row), <8,19,0> 96 (the eight-lane row that
// holds the same reads), seed_band_kernel<48,2,0> 256, score_kernel_v2<32,5,0> 42 -> 48. That leaves 512 - 256 - 48 = 208 for
// the tail: one wavefront of a four-lane configuration (a second one: 288 + 256 + 48 = 592, and the second tier's blocks would
// wait for the slice to end), or two of <8,19> (192). Either way 1024 SIMDs hold 32,768 reads of the tail, its hard upper bound.
// The configuration (HANDBACK_TAIL_G) and the size below the bound are measured: the tail is as long as ONE of its
// wavefronts takes for its 2,000 rows on a SIMD it shares, 1.35 ms for a wavefront of <4,38> and for two of <8,19> — longer than
// the 1.0 ms of the kernels it runs beside — and about half for one wavefront of <8,19>. So: eight lanes, one wavefront per SIMD.
constexpr uint32_t HANDBACK_SIMDS = 1024;                 // 256 CUs x 4
constexpr uint32_t HANDBACK_VGPRS_PER_SIMD = 512;
constexpr uint32_t HANDBACK_VGPRS_BAND = 256;             // seed_band_kernel<48,2,0>
constexpr uint32_t HANDBACK_VGPRS_REMAINDER = 48;         // score_kernel_v2<32,5,0>
constexpr int HANDBACK_TAIL_G = 8;                        // lanes per pair of the tail's configuration: 4 = the class's own, 8 = its <8, C> row
constexpr uint32_t HANDBACK_VGPRS_TAIL = HANDBACK_TAIL_G == 4 ? 144 : 96;
constexpr uint32_t HANDBACK_TAIL_WAVES_PER_SIMD = (HANDBACK_VGPRS_PER_SIMD - HANDBACK_VGPRS_BAND - HANDBACK_VGPRS_REMAINDER) / HANDBACK_VGPRS_TAIL;
static_assert(HANDBACK_TAIL_G == 4 || HANDBACK_TAIL_G == 8, "the register counts above are those of <4,38> and <8,19>");
static_assert(HANDBACK_TAIL_WAVES_PER_SIMD >= 1 &&
                  HANDBACK_TAIL_WAVES_PER_SIMD * HANDBACK_VGPRS_TAIL + HANDBACK_VGPRS_BAND + HANDBACK_VGPRS_REMAINDER <= HANDBACK_VGPRS_PER_SIMD,
              "the second tier's blocks must find registers beside the tail slice");
constexpr uint32_t HANDBACK_WAVE_READS = 2 * 64 / 4;      // reads per wavefront of a four-lane configuration
constexpr uint32_t HANDBACK_TAIL_MAX_READS = HANDBACK_TAIL_WAVES_PER_SIMD * HANDBACK_SIMDS * (2 * 64 / HANDBACK_TAIL_G);  // 32,768
constexpr uint32_t HANDBACK_TAIL_READS = HANDBACK_SIMDS * (2 * 64 / HANDBACK_TAIL_G);  // 16,384: one wavefront per SIMD
static_assert(HANDBACK_TAIL_READS <= HANDBACK_TAIL_MAX_READS, "the tail's bound from the register file");
constexpr uint32_t HANDBACK_HEAD_READS = 0;  // (tried: 32,768, one wavefront of the class's configuration per SIMD)
constexpr uint32_t HANDBACK_ROUND_READS = 3 * HANDBACK_SIMDS * HANDBACK_WAVE_READS;                            // 98,304
// Classes below this many reads plan no slice (their launches and launch logs are today's): the list of a smaller class reaches
// round + slice only if more than 5 % of its reads have no anchor, where the band tiers, not the list, are the long part.
constexpr uint32_t HANDBACK_SLICE_MIN_CLASS = 1u << 21;
// ZSW_DEBUG_SEED_TINY_SLICES: slices at any class size, for the tests — a tail of exactly one block (128 reads) in front of
// which a head of 1 .. 128 reads is cut, and no round kept: lists of 1 .. 127 reads are a head alone, 128 a tail alone, 129 both
// with nothing left to the shared launch, 130 and more all three parts.
constexpr uint32_t HANDBACK_TINY_TAIL_READS = 128, HANDBACK_TINY_HEAD_READS = 128, HANDBACK_TINY_HEAD_MIN = 1;

struct ItemRange {
    uint32_t first, end;
};
struct HandbackSlices {
    ItemRange shared, head, tail;
};
// What the host knows of a call: the most reads each slice takes, the fewest it is worth a launch for, and what the shared launch keeps.
struct HandbackSliceRule {
    uint32_t keep;                 // the shared launch's part never drops below this because of a slice
    uint32_t tail_reads, tail_min;
    uint32_t head_reads, head_min;
    constexpr bool head() const { return head_reads != 0; }
    constexpr bool tail() const { return tail_reads != 0; }
};
// coscheduled: handback_coschedule(cc) holds for the call; own_stream: it runs on the caller's stream (the one-length route — a
// length class of a ragged batch is on a side stream already); no_slices / tiny: ZSW_DEBUG_SEED_NO_SLICES / _TINY_SLICES.
constexpr HandbackSliceRule handback_slice_rule(bool coscheduled, bool own_stream, uint32_t class_reads, bool no_slices, bool tiny) {
    if (!coscheduled || !own_stream || no_slices) return HandbackSliceRule{0u, 0u, 0u, 0u, 0u};
    if (tiny) return HandbackSliceRule{0u, HANDBACK_TINY_TAIL_READS, HANDBACK_TINY_TAIL_READS, HANDBACK_TINY_HEAD_READS, HANDBACK_TINY_HEAD_MIN};
    if (class_reads < HANDBACK_SLICE_MIN_CLASS) return HandbackSliceRule{0u, 0u, 0u, 0u, 0u};
    return HandbackSliceRule{HANDBACK_ROUND_READS, HANDBACK_TAIL_READS, HANDBACK_TAIL_READS, HANDBACK_HEAD_READS, HANDBACK_HEAD_READS};
}
// The three parts of list[0, n0). The tail is cut first (it is worth more: the idle time behind the shared launch is the longer).
constexpr HandbackSlices handback_slices(uint32_t n0, const HandbackSliceRule& r) {
    uint32_t avail = n0 > r.keep ? n0 - r.keep : 0u;
    const uint32_t tail = (r.tail_reads && avail >= r.tail_min) ? (avail < r.tail_reads ? avail : r.tail_reads) : 0u;
    avail -= tail;
    const uint32_t head = (r.head_reads && avail >= r.head_min) ? (avail < r.head_reads ? avail : r.head_reads) : 0u;
    const uint32_t s = n0 - tail - head;
    return HandbackSlices{{0u, s}, {s, s + head}, {s + head, n0}};
}
// The device words a launch reads its range from: bounds[0] = shared.end = head.first, bounds[1] = head.end = tail.first; tail.end
// is n0 itself. (ScoreArgsV2: n_items_dev -> a range's end, first_item_dev -> its first.)
constexpr int HANDBACK_BOUND_WORDS = 2;

}  // namespace zsw
