// zsw_seed_diag.hpp — what the diagonal first tier (seed_diag_kernel, zsw_score_band.hip) derives from zsw_seed.hpp once per
// group of columns instead of once per column. A strip of ONE column is a band of wu + wd + 1 diagonals (zsw_seed.hpp, "banded
// pass", C = 1): after EVERY column the band's top cell joins the paths above the band, on the track seed_exit_is_free names.
// Host model: tests/models/seed_diag.cpp (every column of every layout against seed_exit_is_free itself).
#pragma once
#include "zsw_seed.hpp"

namespace zsw {

// bit i (i < n <= 32) = seed_exit_is_free(k0 + i, ...). Column x is free exactly inside the territory of a k-mer of the mask, the
// columns [c_j - spacer, c_j + K - 1): strides are at least K + spacer, so the territories are disjoint and the first k-mer whose
// last column lies behind x is the only one that can hold x.
ZSW_SEED_HD uint32_t seed_free_bits(int k0, int n, int m, int c0, int stride, int K, int spacer, uint32_t magic, uint32_t mask) {
    uint32_t bits = 0;
    for (int j = seed_started(k0 - K + 1, m, c0, magic); j < m; ++j) {  // the first k-mer whose last column lies behind k0
        const int cj = c0 + j * stride;
        if (cj - spacer >= k0 + n) break;
        if (!((mask >> j) & 1u)) continue;
        const int lo = cj - spacer > k0 ? cj - spacer - k0 : 0, hi = cj + K - 1 < k0 + n ? cj + K - 1 - k0 : n;  // columns [lo, hi) of the group
        if (hi > lo) bits |= (hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
    }
    return bits;
}

// bits [max(t, 0), 32) / bits [0, min(t, 32)): the columns of a group at or behind / before a threshold
ZSW_SEED_HD uint32_t seed_bits_from(int t) { return t >= 32 ? 0u : 0xffffffffu << (t > 0 ? t : 0); }
ZSW_SEED_HD uint32_t seed_bits_below(int t) { return ~seed_bits_from(t); }
ZSW_SEED_HD uint32_t seed_bits_range(int lo, int hi) { return seed_bits_from(lo) & seed_bits_below(hi); }  // bits [max(lo, 0), min(hi, 32))

// The events of a group of columns [k0, k0 + n), n <= 16, without a loop over the k-mers. Which columns a k-mer j occupies depends on
// the read's layout alone, whether it counts on the mask: so a group has the UNMASKED column patterns of the few k-mers that can
// touch it, and a mask picks among them. K-mer j touches the group with the columns [c_j - spacer, c_j + K - 1] (its territory and
// its last column). j0 = the first k-mer whose last column is not left of the group: c_j0 >= k0 - K + 1, so with strides of at
// least K + spacer (seed_layout, wherever a read has a second k-mer) c_(j0+3) - spacer >= k0 + 2 * (K + spacer) + 1 >= k0 + n.
constexpr int SEED_GROUP_KMERS = 3, SEED_GROUP_MAX = 16, SEED_GROUP_MIN_STRIDE = 8;
static_assert(2 * SEED_GROUP_MIN_STRIDE + 1 >= SEED_GROUP_MAX, "a fourth k-mer could touch a group (K + spacer >= 8: K is 8 .. 12; tests/models/seed_diag_events.cpp)");
struct SeedGroupPatterns {
    int j0;
    // bit i, of k-mer j0 + t (all 0 if there is no such k-mer): column k0 + i is its first / its last / one of [c_j, c_j + K - 1) /
    // of its territory [c_j - spacer, c_j + K - 1)
    uint32_t start[SEED_GROUP_KMERS], end[SEED_GROUP_KMERS], inside[SEED_GROUP_KMERS], terr[SEED_GROUP_KMERS];
};
ZSW_SEED_HD SeedGroupPatterns seed_group_patterns(int k0, int n, int m, int c0, int stride, int K, int spacer, uint32_t magic) {
    SeedGroupPatterns g;
    g.j0 = seed_started(k0 - K, m, c0, magic);
    const uint32_t cols = seed_bits_below(n);
#pragma unroll
    for (int t = 0; t < SEED_GROUP_KMERS; ++t) {
        const int j = g.j0 + t;
        const int first = c0 + j * stride - k0, last = first + K - 1;  // relative to the group
        const uint32_t live = j < m ? cols : 0u;
        g.start[t] = seed_bits_range(first, first + 1) & live;
        g.end[t] = seed_bits_range(last, last + 1) & live;
        g.inside[t] = seed_bits_range(first, last) & live;
        g.terr[t] = seed_bits_range(first - spacer, last) & live;
    }
    return g;
}
// the patterns of the k-mers a mask holds (bit j: k-mer j counts; 16 bits): with pat = start / end / inside what seed_strip_events
// returns for the group, with pat = terr what seed_free_bits returns
ZSW_SEED_HD uint32_t seed_group_pick(const uint32_t* pat, int j0, uint32_t mask) {
    const uint32_t b = (mask & 0xffffu) >> j0;  // (j0 <= m <= 16)
    return ((0u - (b & 1u)) & pat[0]) | ((0u - ((b >> 1) & 1u)) & pat[1]) | ((0u - ((b >> 2) & 1u)) & pat[2]);
}

// A walk whose band stays inside the reference: in every column c < lenmax of every group, the five edge words of the kernel's
// group prologue (zsw_seed_diag_body.inc: above, topin, below, exits, yfok) have the column's bit set. Column c of the walk covers
// the rows [dtmin - wu + c, dtmax + c + 1 + wd); with t0 = dtmin - wu + k0, t1 = dtmax + k0 + 1 + wd and c = k0 + u the words say
//   above: t0 + u >= 1          topin: 0 <= t0 + u < R          below: t1 + u < R          exits: below, t1 + u >= 1          yfok: below, t1 + u >= 0
// Each bound is tightest in the first or the last column, so the walk's two corners decide: the first row of column 0 has a row above
// it inside the matrix (dtmin - wu >= 1: above; topin's lower bound with it), and the first row below the band in the last column is
// a row of the reference (dtmax + lenmax + wd < R: below; topin's upper bound with it, as dtmin - wu <= dtmax + wd + 1). exits and
// yfok add dtmax + wd >= 0, which the first condition implies for wu, wd >= 0; it is kept so that the predicate stands without
// that premise. Model: tests/models/seed_diag_interior.cpp (every column's words as the body evaluates them).
ZSW_SEED_HD bool diag_walk_is_interior(int dtmin, int dtmax, int wu, int wd, int lenmax, int R) {
    return dtmin - wu >= 1 && dtmin - wu + lenmax - 1 < R && dtmax + lenmax + wd < R && dtmax + wd >= 0;
}

}  // namespace zsw
