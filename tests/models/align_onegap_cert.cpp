// align_onegap_cert.cpp — host model of the one-gap certificate that lets sw_simd_align's second pass be skipped for a read: the
// read's only optimal alignments have exactly ONE gap run (zoe_amd/csrc/zsw_cert.hpp, compiled here as the classify pass of
// zsw_threepass.hip compiles it; the gapless case: align_gapless_cert.cpp; the independent pieces: align_cert_common.hpp).
//
// For every pair the model finds with plain Gotoh whether both maxima sit in one cell each and where, runs the classify launch of
// cert_decide and, for a deferred read, the sweep launch, and checks every certificate it issues twice: a Gotoh that counts the
// alignments between the two corners must find exactly as many that score S as the certificate found adjacent tied placements
// (a gap inside a homopolymer run: the same alignment shifted along the run — and nothing else), and the oracle's literal
// sw_simd_align must return [qs S][p M][g D|I][m - p M][len - qe S] with p the LAST of them (the walk from the end, backtrack.rs:
// 290-342, tests E == H / F == H before the diagonal) at every listed <T, N> — signed and unsigned 8-, 16- and 32-bit lanes, and
// with the roles swapped as the shared-profile role sees them. Pairs: one indel of 1-5 with few other errors, single indels inside
// homopolymer runs and short repeats (tied placements), a second indel a few bases away (two runs that may score exactly S), a
// second indel farther away (around the bound amax of the two-run search), junk ends; sixteen schemes (gap_extend 0: never certified).
// usage: align_onegap_cert <iterations> <seed>
//
// Also built as a library (-DZSW_MODEL_LIB) for tests/test_gpu_cert.py: zsw_model_cert_verdicts() gives the kernel's own first-pass
// values to the same two launches of cert_decide, zsw_model_cert_corners() the plain-Gotoh maxima and corners of a list of reads.
#include "align_cert_common.hpp"

using namespace certm;

#ifdef ZSW_MODEL_LIB
namespace {
// sequences as residue indices, w: S x S in the kernel's orientation (row = the `reference` of three_pass.rs:21-26)
Scheme index_scheme(const int32_t* w, int S, int go, int ge) {
    Scheme sc;
    sc.name = "lib";
    uint8_t keys[MAX_S];
    for (int i = 0; i < S; ++i) keys[i] = (uint8_t)i;
    sc.map = ByteIndexMap::make(keys, S, 0, false);
    sc.wm.S = S;
    for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) sc.wm.w[i][j] = (int8_t)w[i * S + j];
    sc.go = go;
    sc.ge = ge;
    sc.letters = S;
    return sc;
}

// read i of a batch and the sequence on the other side; shared = 0: `reference` = ref, `query` = read i (run_align), shared = 1:
// `reference` = read i, `query` = ref (run_align_shared)
void sides(const uint8_t* ref, uint32_t ref_len, const uint8_t* reads, const uint64_t* offsets, uint32_t i, int shared, Seq* r, Seq* q) {
    const Seq a(ref, ref + ref_len), b(reads + offsets[i], reads + offsets[i + 1]);
    *r = shared ? b : a;
    *q = shared ? a : b;
}
}  // namespace

extern "C" {
// out[4 i ..]: verdict, parameter, ties, 1 = decided by the sweep launch (zsw_debug_cert_records) from the kernel's first-pass values
int zsw_model_cert_verdicts(const int32_t* w, int S, int go, int ge, const uint8_t* ref, uint32_t ref_len, const uint8_t* reads,
                            const uint64_t* offsets, uint32_t n, int shared, const uint32_t* score, const uint32_t* rs, const uint32_t* re,
                            const uint32_t* qs, const uint32_t* qe, const uint8_t* unique, int32_t* out) {
    const Scheme sc = index_scheme(w, S, go, ge);
    for (uint32_t i = 0; i < n; ++i) {
        Seq r, q;
        sides(ref, ref_len, reads, offsets, i, shared, &r, &q);
        Corners k;
        k.unique = unique[i] != 0;
        k.S = (int)score[i];
        k.rs = (int)rs[i], k.re = (int)re[i], k.qs = (int)qs[i], k.qe = (int)qe[i];
        if (k.unique && (k.re > (int)r.size() || k.qe > (int)q.size())) return 1;
        const Verdict v = certify(r, q, sc, k);
        out[4 * i] = v.r.verdict;
        out[4 * i + 1] = v.r.param;
        out[4 * i + 2] = v.r.ties;
        out[4 * i + 3] = v.swept ? 1 : 0;
    }
    return 0;
}

// out[6 i ..]: both maxima in one cell, S, rs, re, qs, qe (plain Gotoh over the whole matrix and its reverse); certified reads
// (cert[i]): out[6 i] = -1 if the optimal alignments between the corners are not exactly `ties[i]` (gapless: 1)
int zsw_model_cert_corners(const int32_t* w, int S, int go, int ge, const uint8_t* ref, uint32_t ref_len, const uint8_t* reads,
                           const uint64_t* offsets, uint32_t n, int shared, const int32_t* want_alignments, int32_t* out) {
    const Scheme sc = index_scheme(w, S, go, ge);
    for (uint32_t i = 0; i < n; ++i) {
        Seq r, q;
        sides(ref, ref_len, reads, offsets, i, shared, &r, &q);
        const Corners k = corners(r, q, sc);
        out[6 * i] = k.unique ? 1 : 0;
        out[6 * i + 1] = k.S, out[6 * i + 2] = k.rs, out[6 * i + 3] = k.re, out[6 * i + 4] = k.qs, out[6 * i + 5] = k.qe;
        if (k.unique && want_alignments[i] > 0) {
            const Count c = count_optimal(r, q, sc, k.rs, k.re, k.qs, k.qe);
            if (c.best != k.S || c.n != want_alignments[i]) out[6 * i] = -1;
        }
    }
    return 0;
}
}
#else
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
        const int R = rnd(80, 300);
        Seq ref(R);
        for (auto& x : ref) x = base();
        if (rnd(0, 2) == 0) {  // a second copy of a stretch
            const int len = rnd(10, 40), from = rnd(0, R - len), to = rnd(0, R - len);
            for (int i = 0; i < len; ++i) ref[to + i] = ref[from + i];
        }
        for (int h = rnd(0, 3); h > 0; --h) {  // homopolymer / short tandem runs
            const int unit = rnd(1, 3), len = rnd(6, 16), at = rnd(0, R - len);
            for (int i = unit; i < len; ++i) ref[at + i] = ref[at + i - unit];
        }
        for (int k = 0; k < 12; ++k) {
            const int L = rnd(12, 70);
            const int p0 = rnd(0, std::max(0, R - L - 40));
            // the read as a list of edits of ref[p0 ..]: a first indel, and for some kinds a second one
            const int kind = k % 4;
            int at1 = rnd(3, L - 4), len1 = (rnd(0, 1) ? 1 : -1) * (rnd(0, 3) ? 1 : rnd(2, 5));
            if (kind == 1) {  // the first indel inside a homopolymer / tandem run of the reference, if there is one nearby
                for (int t = 0; t < L - 6; ++t) {
                    const int c = (at1 + t) % (L - 6) + 3;
                    if (p0 + c + 2 < R && ref[p0 + c] == ref[p0 + c + 1] && ref[p0 + c + 1] == ref[p0 + c + 2]) {
                        at1 = c + 1;
                        break;
                    }
                }
            }
            int at2 = -1, len2 = 0;
            if (kind == 2) {  // a second indel a few bases away: two runs, some of them at exactly S
                at2 = at1 + rnd(1, 6);
                len2 = (rnd(0, 1) ? 1 : -1) * rnd(1, 3);
            } else if (kind == 3) {  // farther away: around amax
                at2 = at1 + rnd(6, 30);
                len2 = (rnd(0, 1) ? 1 : -1) * rnd(1, 6);
            }
            const int subs = rnd(0, 2);
            Seq q;
            int p = p0;
            for (int i = 0; (int)q.size() < L && p < R; ++i) {
                if (i == at1 || i == at2) {
                    const int len = i == at1 ? len1 : len2;
                    if (len < 0) p += -len;  // a deletion from the read
                    else for (int x = 0; x < len; ++x) q.push_back(base());
                }
                if (p >= R) break;
                q.push_back(ref[p++]);
            }
            while ((int)q.size() < L) q.push_back(base());
            for (int s = 0; s < subs; ++s) {
                const int at = rnd(0, L - 1);
                q[at] = rnd(0, 3) || sc.letters != 4 ? other(q[at]) : 'N';
            }
            if (k % 5 == 1) {  // junk ends: the alignment is clipped
                for (int i = 0; i < rnd(1, 6); ++i) q[i] = base();
                for (int i = 0; i < rnd(1, 6); ++i) q[L - 1 - i] = base();
            }
            if (!check_pair(ref, q, sc, n)) return 1;
        }
    }
    print_tally("align_onegap_cert", n);
    if (n.one_gap * 12 < n.pairs || n.tied * 10 < n.one_gap || n.swept * 20 < n.one_gap) {
        printf("the certificate is vacuous: fewer than a twelfth of the pairs get a one-gap certificate, or hardly any ties or sweeps\n");
        return 1;
    }
    printf("align_onegap_cert OK\n");
    return 0;
}
#endif
