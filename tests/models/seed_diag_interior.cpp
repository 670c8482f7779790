// seed_diag_interior.cpp — host check of diag_walk_is_interior (zsw_seed_diag.hpp), the predicate by which a wavefront of the diagonal
// first tier takes the copy of its column loop that applies no edge mask. Exhaustive over R in {40, 300, 2000}, L in {24, 25, 150,
// 255}, dtmin in [-L - 20, R + 20], dtmax - dtmin in {0, 1}, with the narrow band of the tier (wu = 8, wd = 6):
//   1. wherever the predicate is true, the five edge words of the kernel's group prologue (above, topin, below, exits, yfok), evaluated
//      with seed_bits_from / seed_bits_below exactly as zsw_seed_diag_body.inc evaluates them, have the bit of every column c < L of
//      every group set;
//   2. the predicate is tight: wherever it is false, one of the words lacks a bit in an executed column (so no interior walk is sent
//      through the masked loop for nothing);
//   3. it is not vacuous: false for some dtmin on either side of every R, true for some dtmin wherever a walk fits the reference.
// Prints the fraction of interior walks over the anchors 0 .. R - L of R = 2000, L = 150.
#include <cstdint>
#include <cstdio>

#include "../../zoe_amd/csrc/zsw_seed_diag.hpp"

namespace {

constexpr int GROUP = 16, WU = 8, WD = 6;

// the body's words of the group that starts at column k0, ANDed over the columns the walk executes: all five all-ones there?
bool words_all_ones(int dtmin, int dtmax, int L, int R, bool verbose) {
    const int base = dtmin - WU;
    for (int k0 = 0; k0 < L; k0 += GROUP) {
        const int t0 = base + k0, t1 = dtmax + k0 + 1 + WD;
        const uint32_t above = zsw::seed_bits_from(1 - t0), below = zsw::seed_bits_below(R - t1);
        const uint32_t topin = zsw::seed_bits_from(-t0) & zsw::seed_bits_below(R - t0);
        const uint32_t exits = below & zsw::seed_bits_from(1 - t1), yfok = below & zsw::seed_bits_from(-t1);
        const uint32_t executed = zsw::seed_bits_below(L - k0) & 0xffffu;  // the columns k0 + u < L, u < 16
        const uint32_t words[5] = {above, topin, below, exits, yfok};
        static const char* const names[5] = {"above", "topin", "below", "exits", "yfok"};
        for (int i = 0; i < 5; ++i)
            if ((words[i] & executed) != executed) {
                if (verbose) printf("R %d L %d dtmin %d dtmax %d k0 %d: %s is %08x, executed columns %04x\n", R, L, dtmin, dtmax, k0, names[i], words[i], executed);
                return false;
            }
    }
    return true;
}

}  // namespace

int main() {
    const int Rs[3] = {40, 300, 2000}, Ls[4] = {24, 25, 150, 255};
    long checked = 0, interior = 0;
    for (int R : Rs)
        for (int L : Ls)
            for (int slack = 0; slack <= 1; ++slack) {
                bool false_low = false, false_high = false, any_true = false;
                int first_true = 0, last_true = 0;
                for (int dtmin = -L - 20; dtmin <= R + 20; ++dtmin) {
                    const int dtmax = dtmin + slack;
                    const bool p = zsw::diag_walk_is_interior(dtmin, dtmax, WU, WD, L, R);
                    const bool ones = words_all_ones(dtmin, dtmax, L, R, p);
                    ++checked;
                    if (p && !ones) {
                        printf("the predicate holds, a word does not\n");
                        return 1;
                    }
                    if (!p && ones) {
                        printf("R %d L %d dtmin %d dtmax %d: every word is all-ones, the predicate is false\n", R, L, dtmin, dtmax);
                        return 1;
                    }
                    if (p) {
                        if (!any_true) first_true = dtmin;
                        last_true = dtmin;
                        any_true = true;
                        ++interior;
                    } else if (!any_true) {
                        false_low = true;
                    } else {
                        false_high = true;
                    }
                }
                if (!any_true) {  // no walk of this length fits the reference with its band: false on every side
                    false_high = false_low;
                    if (WU + 1 + L + slack + WD < R) {
                        printf("R %d L %d slack %d: a walk fits, the predicate is never true\n", R, L, slack);
                        return 1;
                    }
                } else if (first_true != WU + 1 || last_true != R - 1 - WD - L - slack) {
                    // the thresholds as the tests on the GPU place their reads: first band row 1, first row below the band R - 1
                    printf("R %d L %d slack %d: interior for dtmin %d .. %d, expected %d .. %d\n", R, L, slack, first_true, last_true, WU + 1, R - 1 - WD - L - slack);
                    return 1;
                }
                if (!false_low || !false_high) {
                    printf("R %d L %d slack %d: the predicate is never false %s the reference\n", R, L, slack, false_low ? "behind" : "before");
                    return 1;
                }
            }
    // the workload's shape: exact anchors 0 .. R - L, lane partners on one diagonal
    int in = 0, all = 0;
    for (int dt = 0; dt <= 2000 - 150; ++dt, ++all) in += zsw::diag_walk_is_interior(dt, dt, WU, WD, 150, 2000) ? 1 : 0;
    printf("interior walks at R 2000, L 150: %d of %d anchors (%.2f %%)\n", in, all, 100.0 * in / all);
    printf("seed_diag_interior OK: %ld walks checked, %ld interior\n", checked, interior);
    return 0;
}
