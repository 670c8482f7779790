// align_gapless_cert.cpp — host model of the gapless certificate that lets sw_simd_align's second pass be skipped for a read
// (zoe_amd/csrc/zsw_cert.hpp, compiled here as the classify pass of zsw_threepass.hip compiles it; the one-gap case:
// align_onegap_cert.cpp; the independent pieces: align_cert_common.hpp).
//
// sw_simd_align's CIGAR depends on the <T, N> striping only where several optimal alignments exist. For every pair
// the model finds with plain Gotoh whether both maxima sit in one cell each and where (what the seeded passes report), runs the
// classify launch of cert_decide and, for a deferred read, the sweep launch, and checks every certificate it issues twice: a Gotoh
// that counts the alignments between the two corners must find exactly one that scores S, and the oracle's literal sw_simd_align
// (oracle/zoe_oracle.hpp, the restated striped.rs:449-598) must return [qs S][n M][len - qe S] with these ranges at every listed
// <T, N> — signed and unsigned (biased matrix) 8-, 16- and 32-bit lanes, and with the roles swapped as the shared-profile role
// sees them. Pairs: copies with few substitutions and N's, an insertion and a deletion of the same length a few bases apart (the
// two-run alternatives the sweeps enumerate, some of them scoring exactly S), substitution counts around the potential's threshold,
// homopolymer runs and repeats; sixteen schemes (asymmetric matrix, three letters, gap_extend 0 and == gap_open among them).
// usage: align_gapless_cert <iterations> <seed>
#include "align_cert_common.hpp"

using namespace certm;

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 400;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const std::vector<Scheme> all = schemes();
    Tally n;
    for (int it = 0; it < iters; ++it) {
        const Scheme& sc = all[it % all.size()];
        const int letters = it % 7 == 0 ? std::min(2, sc.letters) : sc.letters;
        auto base = [&]() { return sc.keys[rnd(0, letters - 1)]; };
        auto other = [&](uint8_t b) {
            uint8_t x = b;
            while (x == b) x = sc.keys[rnd(0, sc.letters - 1)];
            return x;
        };
        const int R = rnd(60, 300);
        Seq ref(R);
        for (auto& x : ref) x = base();
        if (rnd(0, 2) == 0) {  // a second copy of a stretch
            const int len = rnd(10, 40), from = rnd(0, R - len), to = rnd(0, R - len);
            for (int i = 0; i < len; ++i) ref[to + i] = ref[from + i];
        }
        if (rnd(0, 2) == 0) {  // homopolymer / short tandem runs
            const int unit = rnd(1, 3), len = rnd(6, 20), at = rnd(0, R - len);
            for (int i = unit; i < len; ++i) ref[at + i] = ref[at + i - unit];
        }
        for (int k = 0; k < 12; ++k) {
            const int L = rnd(6, 60);
            const int p = rnd(0, R - L);
            Seq q(ref.begin() + p, ref.begin() + p + L);
            const int kind = k % 4;
            if (kind == 0) {  // a few substitutions and N's
                for (int i = 0; i < L; ++i) {
                    const int e = rnd(0, 99);
                    if (e < 4) q[i] = other(q[i]);
                    else if (e < 5 && sc.letters == 4) q[i] = 'N';
                }
            } else if (kind == 1) {  // a deletion and an insertion of the same length a few bases apart: a two-run detour
                const int kk = rnd(1, 3), i = rnd(2, std::max(2, L - 12)), d = rnd(1, 8);
                Seq t(q.begin(), q.begin() + std::min(i, L));
                if (rnd(0, 1)) {  // deletion first
                    for (int j = i + kk; j < std::min(L, i + kk + d); ++j) t.push_back(ref[p + j]);
                    for (int j = 0; j < kk; ++j) t.push_back(base());
                    for (int j = i + kk + d; j < L; ++j) t.push_back(ref[p + j]);
                } else {  // insertion first
                    for (int j = 0; j < kk; ++j) t.push_back(base());
                    for (int j = i; j < std::min(L, i + d); ++j) t.push_back(ref[p + j]);
                    for (int j = i + d + kk; j < L && p + j < R; ++j) t.push_back(ref[p + j]);
                }
                t.resize(L, base());
                q = t;
                for (int s = rnd(0, 2); s > 0; --s) q[rnd(0, L - 1)] = base();
            } else if (kind == 2) {  // exactly s substitutions: around the potential's threshold (3 gap_open / mismatch loss)
                const int s = rnd(1, 6);
                for (int j = 0; j < s; ++j) {
                    const int at = rnd(0, L - 1);
                    q[at] = other(q[at]);
                }
            } else {  // junk ends and now and then an indel (such reads are not gapless)
                for (int i = 0; i < rnd(1, 6); ++i) q[i] = base();
                for (int i = 0; i < rnd(1, 6); ++i) q[L - 1 - i] = base();
                if (rnd(0, 2) == 0) q.erase(q.begin() + rnd(1, L - 2)), q.push_back(base());
            }
            if (!check_pair(ref, q, sc, n)) return 1;
        }
    }
    print_tally("align_gapless_cert", n);
    if (n.gapless * 6 < n.pairs || n.swept * 40 < n.gapless) {
        printf("the certificate is vacuous: fewer than a sixth of the pairs get a gapless one, or hardly any needs the sweeps\n");
        return 1;
    }
    printf("align_gapless_cert OK\n");
    return 0;
}
