// seed_diag_events.cpp — host check of the loop-free group events of the diagonal first tier (zsw_seed_diag.hpp:
// seed_group_patterns / seed_group_pick, what seed_diag_kernel derives once per group of 16 columns) against the loops they
// replace. Exhaustive over the layouts: every read length min_len .. max_len, K = 8 .. 12, spacer 2 .. 4, every group start k0
// (multiples of 16 below the length); per layout the masks 0, all-ones, every single bit and a few hundred random ones.
//   1. the masked start / end / inside bits equal seed_strip_events(k0, 16, ...), the masked territory bits seed_free_bits(k0, 16, ...);
//   2. no k-mer besides j0, j0 + 1, j0 + 2 touches the group (its columns [c_j - spacer, c_j + K - 1] miss [k0, k0 + 16)), and the
//      strides are at least K + spacer wherever a read has more than one k-mer: the bound SEED_GROUP_KMERS rests on;
//   3. the unmasked territory bits equal seed_exit_is_free column by column.
// usage: seed_diag_events <min_len> <max_len> [random masks per layout] [seed]   (SEED_MIN_LEN, SEED_DIAG_MAX_LEN of zsw_score_seed.hpp)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../zoe_amd/csrc/zsw_seed_diag.hpp"

namespace {

constexpr int GROUP = 16;

struct Layout {
    int L, K, spacer, m, stride, c0;
    uint32_t magic;
};

bool fail(const Layout& y, int k0, uint32_t mask, const char* what, uint32_t got, uint32_t want) {
    printf("L %d K %d spacer %d (m %d stride %d c0 %d) k0 %d mask %04x: %s is %04x, want %04x\n", y.L, y.K, y.spacer, y.m, y.stride, y.c0, k0, mask, what, got, want);
    return false;
}

bool check_group(const Layout& y, int k0, const std::vector<uint32_t>& masks) {
    const zsw::SeedGroupPatterns g = zsw::seed_group_patterns(k0, GROUP, y.m, y.c0, y.stride, y.K, y.spacer, y.magic);
    // 2. the k-mers outside j0 .. j0 + 2 stay clear of the group
    if (g.j0 < 0 || g.j0 > y.m) return fail(y, k0, 0, "j0", (uint32_t)g.j0, (uint32_t)y.m);
    for (int j = 0; j < y.m; ++j) {
        if (j >= g.j0 && j < g.j0 + zsw::SEED_GROUP_KMERS) continue;
        const int cj = y.c0 + j * y.stride;
        if (cj - y.spacer < k0 + GROUP && cj + y.K - 1 >= k0) return fail(y, k0, 0, "a k-mer outside the three touches the group: j", (uint32_t)j, (uint32_t)g.j0);
    }
    // 3. territories, column by column
    uint32_t terr = 0;
    for (int t = 0; t < zsw::SEED_GROUP_KMERS; ++t) {
        if (terr & g.terr[t]) return fail(y, k0, 0, "territories overlap", terr, g.terr[t]);
        terr |= g.terr[t];
        if ((g.start[t] | g.end[t] | g.inside[t] | g.terr[t]) >> GROUP) return fail(y, k0, 0, "bits beyond the group", g.start[t] | g.end[t] | g.inside[t] | g.terr[t], 0);
    }
    for (int i = 0; i < GROUP; ++i) {
        const bool want = zsw::seed_exit_is_free(k0 + i, y.m, y.c0, y.stride, y.K, y.spacer, y.magic, 0xffffu);
        if ((((terr >> i) & 1u) != 0) != want) return fail(y, k0, 0xffffu, "territory bit (index, seed_exit_is_free)", (uint32_t)i, (uint32_t)want);
    }
    // 1. the masked events
    for (const uint32_t mask : masks) {
        const zsw::SeedStripEvents e = zsw::seed_strip_events(k0, GROUP, y.m, y.c0, y.stride, y.K, y.magic, mask);
        const uint32_t fr = zsw::seed_free_bits(k0, GROUP, y.m, y.c0, y.stride, y.K, y.spacer, y.magic, mask);
        const uint32_t s = zsw::seed_group_pick(g.start, g.j0, mask), en = zsw::seed_group_pick(g.end, g.j0, mask);
        const uint32_t in = zsw::seed_group_pick(g.inside, g.j0, mask), te = zsw::seed_group_pick(g.terr, g.j0, mask);
        if (s != e.start) return fail(y, k0, mask, "start", s, e.start);
        if (en != e.end) return fail(y, k0, mask, "end", en, e.end);
        if (in != e.inside) return fail(y, k0, mask, "inside", in, e.inside);
        if (te != fr) return fail(y, k0, mask, "free", te, fr);
        for (int i = 0; i < GROUP; ++i) {
            const bool want = zsw::seed_exit_is_free(k0 + i, y.m, y.c0, y.stride, y.K, y.spacer, y.magic, mask);
            if ((((te >> i) & 1u) != 0) != want) return fail(y, k0, mask, "free bit (index, seed_exit_is_free)", (uint32_t)i, (uint32_t)want);
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        printf("usage: seed_diag_events <min_len> <max_len> [random masks per layout] [seed]\n");
        return 2;
    }
    const int min_len = atoi(argv[1]), max_len = atoi(argv[2]);
    const int n_random = argc > 3 ? atoi(argv[3]) : 300;
    std::mt19937_64 rng(argc > 4 ? strtoull(argv[4], nullptr, 10) : 1);
    static_assert(zsw::SEED_GROUP_KMERS == 3, "the three patterns of a group");
    long long groups = 0, events = 0;
    for (int K = 8; K <= 12; ++K)
        for (int spacer = 2; spacer <= 4; ++spacer)
            for (int L = min_len; L <= max_len; ++L) {
                Layout y;
                y.L = L;
                y.K = K;
                y.spacer = spacer;
                zsw::seed_layout(L, K, spacer, &y.m, &y.stride, &y.c0);
                y.magic = zsw::seed_div_magic(y.stride);
                if (y.m > 1 && y.stride < K + spacer) {
                    printf("L %d K %d spacer %d: stride %d is below K + spacer\n", L, K, spacer, y.stride);
                    return 1;
                }
                std::vector<uint32_t> masks = {0u, 0xffffu};
                for (int b = 0; b < 16; ++b) masks.push_back(1u << b);
                for (int r = 0; r < n_random; ++r) masks.push_back((uint32_t)rng() & 0xffffu);
                for (int k0 = 0; k0 < L; k0 += GROUP) {
                    if (!check_group(y, k0, masks)) return 1;
                    ++groups;
                    events += (long long)masks.size();
                }
            }
    printf("seed_diag_events OK: %lld groups, %lld masked groups\n", groups, events);
    return 0;
}
