// align_cert_common.hpp — the independent half of the alignment certificate models (align_gapless_cert.cpp, align_onegap_cert.cpp):
// scoring schemes, plain Gotoh for the maxima and their cells, a Gotoh that counts the optimal alignments between two corners, the
// two launches of the classify pass around zsw_cert.hpp's cert_decide, and the oracle's literal sw_simd_align at every listed <T, N>.
// The certificate itself is zoe_amd/csrc/zsw_cert.hpp, the header the kernel compiles; nothing here restates it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../oracle/zoe_oracle.hpp"
#ifndef ZSW_CERT_HEADER
#define ZSW_CERT_HEADER "../../zoe_amd/csrc/zsw_cert.hpp"
#endif
#include ZSW_CERT_HEADER

namespace certm {

using namespace zor;
using Seq = std::vector<uint8_t>;

struct Scheme {
    const char* name;
    ByteIndexMap map;
    WeightMatrixI8 wm;  // rows = reference residue, as in striped.rs
    int go, ge;         // positive magnitudes
    int letters;        // residues the generators draw from (keys[0 .. letters - 1])
    uint8_t keys[5];
    int maxw() const {  // zsw_cert.hpp's helper over the S x S matrix, as certificate_pass calls it
        std::vector<int32_t> w;
        for (int i = 0; i < wm.S; ++i)
            for (int j = 0; j < wm.S; ++j) w.push_back(wm.w[i][j]);
        return zsw::cert_maxw(w.data(), wm.S);
    }
    long w(uint8_t a, uint8_t b) const { return wm.w[map.to_index(a)][map.to_index(b)]; }
};

inline Scheme dna(const char* name, int match, int mismatch, int go, int ge, int letters = 4) {
    Scheme s;
    s.name = name;
    const uint8_t k[5] = {'A', 'C', 'G', 'T', 'N'};
    std::copy(k, k + 5, s.keys);
    s.map = ByteIndexMap::make(k, 5, 'N', true);
    s.wm = WeightMatrixI8::make(s.map, (int8_t)match, (int8_t)mismatch, 'N');
    s.go = go;
    s.ge = ge;
    s.letters = letters;
    return s;
}

// an asymmetric 5 x 5 matrix: the largest weight (5) is on one residue's diagonal only, and w[x][y] != w[y][x]
inline Scheme asymmetric(int go, int ge) {
    Scheme s = dna("asym", 1, -1, go, ge);
    const int8_t m[5][5] = {{3, -2, -4, -1, 0}, {-3, 4, -2, -5, 0}, {-1, -3, 3, -2, 0}, {-4, -1, -3, 5, 0}, {0, 0, 0, 0, -1}};
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) s.wm.w[i][j] = m[i][j];
    s.name = "asym";
    return s;
}

// a three-letter alphabet with its own map (S = 3)
inline Scheme three_letters(int match, int mismatch, int go, int ge) {
    Scheme s;
    s.name = "acg";
    const uint8_t k[5] = {'A', 'C', 'G', 'A', 'A'};
    std::copy(k, k + 5, s.keys);
    s.map = ByteIndexMap::make(k, 3, 'A', true);
    s.wm = WeightMatrixI8::make(s.map, (int8_t)match, (int8_t)mismatch, -1);
    s.go = go;
    s.ge = ge;
    s.letters = 3;
    return s;
}

inline std::vector<Scheme> schemes() {
    return {dna("2/-5,10/1", 2, -5, 10, 1), dna("1/-1,2/1", 1, -1, 2, 1), dna("3/-2,5/1", 3, -2, 5, 1), dna("1/-3,5/2", 1, -3, 5, 2),
            dna("5/-4,8/1", 5, -4, 8, 1), dna("2/-2,3/3", 2, -2, 3, 3), dna("4/-6,12/2", 4, -6, 12, 2), dna("2/-10,10/1", 2, -10, 10, 1),
            dna("1/-1,1/1", 1, -1, 1, 1), dna("3/-1,1/0", 3, -1, 1, 0),
            dna("2/-10,3/1", 2, -10, 3, 1),   // cheap gaps, expensive mismatches
            dna("5/-9,2/2", 5, -9, 2, 2),     // gap_extend == gap_open
            dna("3/-3,4/0", 3, -3, 4, 0),     // gap_extend == 0: gapless certificates only
            dna("9/-20,20/5", 9, -20, 20, 5), // a large match
            asymmetric(6, 1), three_letters(2, -3, 5, 1)};
}

struct Cells {
    int best = 0, n = 0, r = -1, c = -1;
};

// plain Gotoh; the maximum, how many cells hold it, and one of them
inline Cells gotoh(const Seq& a, const Seq& b, const Scheme& sc) {
    const int R = (int)a.size(), L = (int)b.size();
    std::vector<int> H(L + 1, 0), E(L + 1, 0);
    Cells out;
    for (int r = 0; r < R; ++r) {
        int diag = 0, f = 0;
        for (int c = 1; c <= L; ++c) {
            const int e = std::max(std::max(E[c] - sc.ge, H[c] - sc.go), 0);
            f = std::max(std::max(f - sc.ge, H[c - 1] - sc.go), 0);
            const int h = std::max(std::max(diag + (int)sc.w(a[r], b[c - 1]), e), std::max(f, 0));
            diag = H[c];
            H[c] = h;
            E[c] = e;
            if (h > out.best) {
                out.best = h;
                out.n = 1;
                out.r = r;
                out.c = c - 1;
            } else if (h == out.best && h > 0) {
                ++out.n;
            }
        }
    }
    return out;
}

// Both maxima in one cell each, and the corners: what the forward and the reversed seeded pass report (mode 3).
struct Corners {
    bool unique = false;
    int S = 0, rs = 0, re = 0, qs = 0, qe = 0;
};

inline Corners corners(const Seq& ref, const Seq& q, const Scheme& sc) {
    Corners k;
    const Cells fwd = gotoh(ref, q, sc);
    if (fwd.best == 0 || fwd.n != 1) return k;
    const Seq rref(ref.rbegin(), ref.rend()), rq(q.rbegin(), q.rend());
    const Cells rev = gotoh(rref, rq, sc);
    if (rev.best != fwd.best || rev.n != 1) return k;
    k.unique = true;
    k.S = fwd.best;
    k.re = fwd.r + 1;
    k.qe = fwd.c + 1;
    k.rs = (int)ref.size() - 1 - rev.r;
    k.qs = (int)q.size() - 1 - rev.c;
    return k;
}

// Alignments from the pair (rs, qs) to the pair (re - 1, qe - 1) (every alignment that scores S, when both maxima sit in one cell):
// their best score and how many reach it (saturating). Three states — pair, deletion run, insertion run; a run opens from a pair or
// from a run of the other kind — so that every alignment is one path.
struct Count {
    long best;
    long n;
};

inline Count count_optimal(const Seq& ref, const Seq& q, const Scheme& sc, int rs, int re, int qs, int qe) {
    const long NEG = -(1l << 40), CAP = 1l << 20;
    const int R = re - rs, L = qe - qs;
    struct Cell {
        long s[3];
        long n[3];
    };
    std::vector<Cell> D((size_t)R * L);
    auto at = [&](int i, int j) -> Cell& { return D[(size_t)i * L + j]; };
    auto merge = [&](long& s, long& n, long s2, long n2) {
        if (n2 == 0 || s2 <= NEG / 2) return;
        if (s2 > s) {
            s = s2;
            n = n2;
        } else if (s2 == s) {
            n = std::min(CAP, n + n2);
        }
    };
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < L; ++j) {
            Cell& c = at(i, j);
            for (int t = 0; t < 3; ++t) c.s[t] = NEG, c.n[t] = 0;
            const long w = sc.w(ref[rs + i], q[qs + j]);
            if (i == 0 && j == 0) {
                c.s[0] = w;
                c.n[0] = 1;
            } else if (i > 0 && j > 0) {
                const Cell& p = at(i - 1, j - 1);
                for (int t = 0; t < 3; ++t) merge(c.s[0], c.n[0], p.s[t] + w, p.n[t]);
            }
            if (i > 0) {  // deletion: the run consumes reference rows
                const Cell& p = at(i - 1, j);
                merge(c.s[1], c.n[1], p.s[0] - sc.go, p.n[0]);
                merge(c.s[1], c.n[1], p.s[2] - sc.go, p.n[2]);
                merge(c.s[1], c.n[1], p.s[1] - sc.ge, p.n[1]);
            }
            if (j > 0) {
                const Cell& p = at(i, j - 1);
                merge(c.s[2], c.n[2], p.s[0] - sc.go, p.n[0]);
                merge(c.s[2], c.n[2], p.s[1] - sc.go, p.n[1]);
                merge(c.s[2], c.n[2], p.s[2] - sc.ge, p.n[2]);
            }
        }
    const Cell& e = at(R - 1, L - 1);
    return Count{e.n[0] ? e.s[0] : NEG, e.n[0]};
}

// The classify launch (defer) and, for the reads it defers, the sweep launch — as zsw_threepass.hip runs them.
struct Verdict {
    zsw::CertResult r;
    bool swept = false;
};

inline Verdict certify(const Seq& ref, const Seq& q, const Scheme& sc, const Corners& k) {
    const zsw::CertScheme cs{(long long)sc.maxw(), (long long)sc.go, (long long)sc.ge};
    auto wt = [&](uint32_t i, uint32_t j) -> int32_t { return (int32_t)sc.w(ref[k.rs + i], q[k.qs + j]); };
    auto diag = [&]() -> int64_t {
        int64_t s = 0;
        for (int t = 0; t < k.re - k.rs; ++t) s += wt(t, t);
        return s;
    };
    Verdict v;
    v.r = zsw::cert_decide(wt, diag, k.unique, k.rs, k.re, k.qs, k.qe, (uint32_t)k.S, cs, true);
    if (v.r.deferred) {
        v.r = zsw::cert_decide(wt, diag, k.unique, k.rs, k.re, k.qs, k.qe, (uint32_t)k.S, cs, false);
        v.swept = true;
    }
    return v;
}

// The certified alignment in forward order: [qs S][p M][g D|I][m - p M][len - qe S] (gapless: p = 0, g = 0).
inline AlignmentStates want_states(size_t clip5, int p, int g, uint8_t op, int m, size_t clip3) {
    AlignmentStates want;
    want.soft_clip(clip5);
    if (p) want.add_ciglet({(size_t)p, 'M'});
    if (g) want.add_ciglet({(size_t)g, op});
    want.add_ciglet({(size_t)(m - p), 'M'});
    want.soft_clip(clip3);
    return want;
}

inline ProfileWeights weights(const Scheme& sc, bool is_signed, bool transposed) {
    WeightMatrixI8 m = sc.wm;
    if (transposed)
        for (int i = 0; i < m.S; ++i)
            for (int j = 0; j < m.S; ++j) m.w[i][j] = sc.wm.w[j][i];
    return ProfileWeights::from(m, is_signed);  // unsigned widths: the biased matrix (to_biased_matrix)
}

// The oracle's literal sw_simd_align<T, N> must return the certified alignment. swapped: the shared-profile role — the profile is
// striped over the reference-side sequence with the matrix transposed, the read supplies the rows; deletions and insertions trade
// places and the clipped ends are those of the long sequence.
template <typename T, int N>
bool literal_returns(const Seq& ref, const Seq& q, const Scheme& sc, const Corners& k, int p, int g, uint8_t op, bool swapped) {
    const bool sgn = std::is_signed<T>::value;
    const ProfileWeights pw = weights(sc, sgn, swapped);
    const int m = std::min(k.re - k.rs, k.qe - k.qs);
    Maybe<Alignment> a;
    AlignmentStates want;
    if (!swapped) {
        auto prof = StripedProfile<T, N>::make(q.data(), q.size(), pw, sc.map, -sc.go, -sc.ge);
        a = sw_simd_align<T, N>(ref.data(), ref.size(), prof);
        want = want_states((size_t)k.qs, p, g, op, m, q.size() - (size_t)k.qe);
    } else {
        auto prof = StripedProfile<T, N>::make(ref.data(), ref.size(), pw, sc.map, -sc.go, -sc.ge);
        a = sw_simd_align<T, N>(q.data(), q.size(), prof);
        want = want_states((size_t)k.rs, p, g, op == 'D' ? 'I' : 'D', m, ref.size() - (size_t)k.re);
    }
    if (a.status != SOME) return a.status == OVERFLOWED;  // (an overflowing width answers at the next one)
    const int rs = swapped ? k.qs : k.rs, re = swapped ? k.qe : k.re, qs = swapped ? k.rs : k.qs, qe = swapped ? k.re : k.qe;
    return (int)a.value.score == k.S && (int)a.value.ref_start == rs && (int)a.value.ref_end == re && (int)a.value.query_start == qs &&
           (int)a.value.query_end == qe && a.value.states == want;
}

inline bool literal_all(const Seq& ref, const Seq& q, const Scheme& sc, const Corners& k, int p, int g, uint8_t op) {
#ifdef ZSW_CERT_FEW_WIDTHS  // (the mutation runs of tests/test_align_models.py: shorter compilation)
    return literal_returns<int16_t, 16>(ref, q, sc, k, p, g, op, false) && literal_returns<int16_t, 8>(ref, q, sc, k, p, g, op, true);
#else
    return literal_returns<int16_t, 2>(ref, q, sc, k, p, g, op, false) && literal_returns<int16_t, 4>(ref, q, sc, k, p, g, op, false) &&
           literal_returns<int16_t, 8>(ref, q, sc, k, p, g, op, false) && literal_returns<int16_t, 16>(ref, q, sc, k, p, g, op, false) &&
           literal_returns<int16_t, 32>(ref, q, sc, k, p, g, op, false) && literal_returns<int16_t, 64>(ref, q, sc, k, p, g, op, false) &&
           literal_returns<int8_t, 16>(ref, q, sc, k, p, g, op, false) && literal_returns<int8_t, 32>(ref, q, sc, k, p, g, op, false) &&
           literal_returns<uint8_t, 16>(ref, q, sc, k, p, g, op, false) && literal_returns<uint8_t, 32>(ref, q, sc, k, p, g, op, false) &&
           literal_returns<uint16_t, 4>(ref, q, sc, k, p, g, op, false) && literal_returns<uint16_t, 16>(ref, q, sc, k, p, g, op, false) &&
           literal_returns<uint32_t, 8>(ref, q, sc, k, p, g, op, false) && literal_returns<int32_t, 8>(ref, q, sc, k, p, g, op, false) &&
           literal_returns<int16_t, 4>(ref, q, sc, k, p, g, op, true) && literal_returns<int16_t, 16>(ref, q, sc, k, p, g, op, true) &&
           literal_returns<int16_t, 64>(ref, q, sc, k, p, g, op, true) && literal_returns<int8_t, 32>(ref, q, sc, k, p, g, op, true) &&
           literal_returns<uint16_t, 16>(ref, q, sc, k, p, g, op, true);
#endif
}

inline void print_pair(const Seq& ref, const Seq& q) {
    printf("  ref  ");
    for (uint8_t x : ref) putchar(x);
    printf("\n  read ");
    for (uint8_t x : q) putchar(x);
    printf("\n");
}

// Checks one pair: returns false (after printing why) if a certificate is wrong. The tallies go to `n`.
struct Tally {
    long pairs = 0, unique = 0, gapless = 0, one_gap = 0, tied = 0, swept = 0, by_verdict[8] = {0};
};

inline bool check_pair(const Seq& ref, const Seq& q, const Scheme& sc, Tally& n) {
    ++n.pairs;
    const Corners k = corners(ref, q, sc);
    const Verdict v = certify(ref, q, sc, k);
    ++n.by_verdict[v.r.verdict & 7];
    if (!k.unique) return v.r.verdict == zsw::CERT_NOT_UNIQUE || (printf("verdict %d without unique maxima\n", v.r.verdict), false);
    ++n.unique;
    if (v.r.verdict != zsw::CERT_GAPLESS && v.r.verdict != zsw::CERT_ONE_GAP) return true;
    const int rlen = k.re - k.rs, qlen = k.qe - k.qs;
    const bool gapless = v.r.verdict == zsw::CERT_GAPLESS;
    const int g = std::abs(rlen - qlen), p = gapless ? 0 : v.r.param;
    const uint8_t op = rlen > qlen ? 'D' : 'I';
    (gapless ? n.gapless : n.one_gap) += 1;
    if (v.swept) ++n.swept;
    if (!gapless && v.r.ties > 1) ++n.tied;
    const Count c = count_optimal(ref, q, sc, k.rs, k.re, k.qs, k.qe);
    const long want_n = gapless ? 1 : v.r.ties;
    const bool ok_count = c.best == k.S && c.n == want_n;
    const bool ok_lit = ok_count && literal_all(ref, q, sc, k, p, g, op);
    if (ok_count && ok_lit) return true;
    printf("%s certificate (verdict %d, parameter %d, ties %d, %s launch) is wrong: %s; S %d ref [%d,%d) query [%d,%d) scheme %s\n",
           gapless ? "gapless" : "one-gap", v.r.verdict, v.r.param, v.r.ties, v.swept ? "sweep" : "classify",
           !ok_count ? "the optimal alignments between the corners are not the certified ones" : "the literal sw_simd_align returns another alignment",
           k.S, k.rs, k.re, k.qs, k.qe, sc.name);
    if (!ok_count) printf("  best score between the corners %ld, reached by %ld alignments (certificate: %ld)\n", c.best, c.n, want_n);
    print_pair(ref, q);
    return false;
}

inline void print_tally(const char* model, const Tally& n) {
    printf("%s: pairs %ld, both maxima in one cell %ld, gapless certified %ld, one-gap certified %ld (tied placements %ld), decided by the "
           "sweep launch %ld; verdicts", model, n.pairs, n.unique, n.gapless, n.one_gap, n.tied, n.swept);
    for (int i = 0; i < 8; ++i) printf(" %ld", n.by_verdict[i]);
    printf("\n");
}

}  // namespace certm
