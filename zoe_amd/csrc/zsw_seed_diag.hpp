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

}  // namespace zsw
