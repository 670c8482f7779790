// handback_plan.cpp — host check of the launch plan for the reads the seeded pass hands back (zoe_amd/csrc/zsw_handback.hpp, the
// text seed_items of zsw_score.hip compiles). The list's length exists only on the device, so up to three gated launches of
// score_kernel_v2 are queued and the count picks the one that runs. Claim: for every class (longest read, first-fit configuration,
// n_items reads) and every count 0 <= count <= n_items EXACTLY ONE planned launch has lo <= count < hi; its grid covers `count`
// reads and its G * C columns hold the longest read. A count that no gate holds leaves its reads unscored, two gates score them twice.
// Also with score tables that cannot be built for some lane counts (the range then falls to a later launch).
//
// usage: handback_plan <rule> <n_ascending> <G,C> <G,C> ...   (the list of zsw_score_v2.hpp, in its order)
// rule `plan`: handback_plan as shipped. rule `strict`: the same loop with the comparison it had before — a range is launched only
// if n_items > lo, not n_items >= lo — to show that the claim tells the two apart. Prints one line per violated (length, n_items,
// count, failing-tables set), then the number of violations.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zoe_amd/csrc/zsw_handback.hpp"

using namespace zsw;

namespace {

// the loop before handback_plan existed: `lo < n_items` where the plan has `lo <= n_items`
template <class TablesOk>
int strict_plan(const StripCfg* cfgs, int n_cfgs, uint32_t longest, int g, int c, uint32_t n_items, TablesOk tables_ok, HandbackLaunch* out) {
    int n = 0;
    uint32_t lo = 0;
    for (int k = 0; k < 3; ++k) {
        const uint32_t hi = k < 2 ? HANDBACK_CUTS[k] : 0xffffffffu;
        int g2 = g, c2 = c;
        const bool other = k < 2 && lo < n_items && strip_config_for_batch(cfgs, n_cfgs, longest, HANDBACK_PROBE[k], &g2, &c2) && g2 != g;
        if (other) {
            if (!tables_ok(g2)) continue;
        } else if (k < 2) {
            continue;
        }
        if (lo < n_items) out[n++] = other ? HandbackLaunch{lo, hi, g2, c2, std::min(n_items, hi), true} : HandbackLaunch{lo, hi, g, c, n_items, false};
        lo = hi;
    }
    return n;
}

int lanes_bit(int G) { return G == 4 ? 1 : G == 8 ? 2 : G == 16 ? 4 : G == 32 ? 8 : 16; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const bool strict = std::strcmp(argv[1], "strict") == 0;
    const int n_ascending = std::atoi(argv[2]);
    std::vector<StripCfg> cfgs;
    for (int i = 3; i < argc; ++i) {
        StripCfg c{};
        if (std::sscanf(argv[i], "%d,%d", &c.G, &c.C) != 2) return 2;
        cfgs.push_back(c);
    }
    const int n_cfgs = (int)cfgs.size();
    if (n_ascending < 1 || n_ascending > n_cfgs) return 2;
    const uint32_t sizes[] = {1, 2, 1023, 49151, 49152, 49153, 327679, 327680, 327681, 1000000};
    const uint32_t marks[] = {49151, 49152, 49153, 327679, 327680, 327681};
    long checks = 0, violations = 0;
    for (uint32_t len = 24; len <= 2432; ++len) {
        int g = 0, c = 0;
        if (!strip_config_first_fit(cfgs.data(), n_ascending, len, &g, &c)) {
            std::printf("no configuration holds %u columns\n", len);
            return 1;
        }
        for (uint32_t n : sizes) {
            std::vector<uint32_t> counts = {1, n - 1, n};
            for (uint32_t m : marks) counts.push_back(m);
            for (int fail = 0; fail < 32; ++fail) {  // lane counts (4, 8, 16, 32, 64: one bit each) whose tables cannot be built
                HandbackLaunch plan[HANDBACK_MAX_LAUNCHES + 1];
                int asked = 0;
                auto tables_ok = [&](int G) {
                    ++asked;
                    return (fail & lanes_bit(G)) == 0;
                };
                const int np = strict ? strict_plan(cfgs.data(), n_cfgs, len, g, c, n, tables_ok, plan)
                                      : handback_plan(cfgs.data(), n_cfgs, len, g, c, n, tables_ok, plan);
                bool shape = np <= HANDBACK_MAX_LAUNCHES && asked <= 2;
                int built = 0;
                for (int k = 0; k < np; ++k) {  // the gates ascend without overlap; only the class's configuration runs on the pass's own tables
                    shape = shape && plan[k].lo < plan[k].hi && (k == 0 || plan[k - 1].hi <= plan[k].lo) && plan[k].own_tables == (plan[k].G != g);
                    shape = shape && (plan[k].own_tables ? (fail & lanes_bit(plan[k].G)) == 0 : plan[k].C == c);
                    built += plan[k].own_tables;
                }
                if (!shape) {
                    std::printf("SHAPE len %u n %u fail %d: %d launches, %d tables of %d asked for\n", len, n, fail, np, built, asked);
                    ++violations;
                }
                for (uint32_t count : counts) {
                    if (count > n) continue;
                    ++checks;
                    int taken = 0;
                    bool fits = true;
                    for (int k = 0; k < np; ++k) {
                        if (plan[k].lo <= count && count < plan[k].hi) {
                            ++taken;
                            fits = fits && plan[k].grid_items >= count && (uint32_t)(plan[k].G * plan[k].C) >= len;
                        }
                    }
                    if (taken != 1 || !fits) {
                        std::printf("VIOLATION len %u n %u count %u fail %d taken %d fits %d\n", len, n, count, fail, taken, (int)fits);
                        ++violations;
                    }
                }
            }
        }
    }
    std::printf("handback_plan %s: %ld checks, %ld violations\n", argv[1], checks, violations);
    return 0;
}
