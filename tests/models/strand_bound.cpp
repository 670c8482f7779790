// strand_bound.cpp — host model of the strand-aware score pass (zoe_amd/csrc/zsw_strand.hip). It compiles the header the kernels
// use (zsw_seed.hpp: seed_whole_bound, seed_strand_settled) and checks, with plain integers against the full Gotoh matrix:
//   W  no local alignment of a sequence against the reference scores more than seed_whole_bound().u — for BOTH orientations of
//      every read (the read as given and its reverse complement);
//   R  the decision rule: the strand with more support of the anchor vote runs first (ties: forward); whenever
//      seed_strand_settled lets the other strand go unscored, the answer of the contract (the forward result unless the reverse
//      one ranks strictly higher, by the two full matrices) is the first strand with its score.
// Reads: copies with substitutions / indels / N, reverse-strand copies, chimeras of both strands, reads over inverted repeats
// and palindromic k-mers, reads hanging over the reference's ends, random reads, reads of 1 to 30 bases, and structured cases
// whose columns between two sampled k-mers have no potential (the run >= lambda rule); references with N runs of one to five;
// small K so that chance occurrences are common.
// usage: strand_bound <iterations> <seed>            the checks
//        strand_bound report <reads> <seed>          share of 150-base reads settled per divergence rate (K = 8, 2 kb, 2/-5, -10/-1)
// -DZSW_MODEL_LIB: no main; zsw_model_strand_batch() returns what the kernel stores per read (tests/test_gpu_strands.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#ifdef ZSW_SEED_HEADER
#include ZSW_SEED_HEADER
#else
#include "../../zoe_amd/csrc/zsw_seed.hpp"
#endif

namespace {

using zsw::SeedParams;

struct Scheme {
    int S;
    std::vector<int32_t> w;  // S x S, row = reference residue
    int go, ge;
};

Scheme dna(int match, int mismatch, int n_score, int go, int ge) {
    Scheme s;
    s.S = 5;
    s.w.assign(25, 0);
    for (int x = 0; x < 4; ++x)
        for (int q = 0; q < 4; ++q) s.w[x * 5 + q] = x == q ? match : mismatch;
    for (int x = 0; x < 5; ++x) s.w[x * 5 + 4] = s.w[4 * 5 + x] = n_score;
    s.go = go;
    s.ge = ge;
    return s;
}

// the maximum of the full Gotoh matrix (0 if no cell is positive)
int gotoh(const int32_t* w, int S, int go, int ge, const uint8_t* ref, int R, const uint8_t* q, int L) {
    constexpr int NEG = -(1 << 28);
    std::vector<int> Hp(L + 1, 0), Ep(L + 1, NEG), H(L + 1, 0), E(L + 1, NEG);
    int best = 0;
    for (int r = 0; r < R; ++r) {
        int f = NEG;
        H[0] = 0;
        for (int c = 1; c <= L; ++c) {
            E[c] = std::max(Ep[c] - ge, Hp[c] - go);
            f = std::max(f - ge, H[c - 1] - go);
            int h = Hp[c - 1] + w[ref[r] * S + q[c - 1]];
            h = std::max(std::max(h, 0), std::max(E[c], f));
            H[c] = h;
            best = std::max(best, h);
        }
        std::swap(H, Hp);
        std::swap(E, Ep);
    }
    return best;
}

struct Whole {
    zsw::SeedWhole f, r;
    int first;
};

// what the strand pass derives from one read: q as residue indices, comp[] = residue index of the complement
Whole whole_of(const SeedParams& p, const std::vector<uint32_t>& table, const uint8_t* q, int L, const uint8_t* comp, int min_len) {
    auto look = [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
        *f1 = table[2 * (size_t)code];
        *l1 = table[2 * (size_t)code + 1];
    };
    Whole o;
    o.f = zsw::seed_whole_bound(p, L, min_len, [&](int c) { return zsw::seed_cell(p, (int)q[c]); }, look);
    o.r = zsw::seed_whole_bound(p, L, min_len, [&](int c) { return zsw::seed_cell(p, (int)comp[q[L - 1 - c]]); }, look);
    o.first = o.r.support > o.f.support ? 1 : 0;
    return o;
}

struct Counters {
    long reads = 0, settled = 0, both = 0, bound_hit = 0;
};

const uint8_t COMP5[32] = {3, 2, 1, 0, 4};

std::vector<uint8_t> revcomp(const std::vector<uint8_t>& q) {
    std::vector<uint8_t> r(q.rbegin(), q.rend());
    for (auto& x : r) x = COMP5[x];
    return r;
}

bool check_read(const Scheme& s, const SeedParams& p, const std::vector<uint32_t>& table, const std::vector<uint8_t>& ref,
                const std::vector<uint8_t>& q, int min_len, Counters* cnt) {
    const int R = (int)ref.size(), L = (int)q.size();
    const std::vector<uint8_t> rc = revcomp(q);
    const Whole wh = whole_of(p, table, q.data(), L, COMP5, min_len);
    const int tf = gotoh(s.w.data(), s.S, s.go, s.ge, ref.data(), R, q.data(), L);
    const int tr = gotoh(s.w.data(), s.S, s.go, s.ge, ref.data(), R, rc.data(), L);
    ++cnt->reads;
    bool ok = true;
    // seed_whole_sweep restates seed_read's column sweep: the two must look up the same k-mers and add up the same potential
    // (-DZSW_STRAND_NO_TWIN_CHECK: the mutant runs, where claims W and R themselves have to catch a weakened sweep)
#ifndef ZSW_STRAND_NO_TWIN_CHECK
    if (L >= min_len) {
        std::vector<uint32_t> looked;
        const zsw::SeedRead sr = zsw::seed_read(p, L, [&](int c) { return zsw::seed_cell(p, (int)q[c]); }, [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
            looked.push_back(code);
            *f1 = *l1 = 0;
        });
        zsw::SeedSweep sw;
        zsw::seed_whole_sweep(p, L, min_len, [&](int c) { return zsw::seed_cell(p, (int)q[c]); }, &sw);
        bool same = sr.t_all == sw.t_all && (int)looked.size() == zsw::SEED_MAX_KMERS;
        for (int j = 0; same && j < zsw::SEED_MAX_KMERS; ++j) same = looked[j] == (sw.usable[j] ? sw.codes[j] : 0u);
        if (!same) {
            printf("the sweeps of seed_read and seed_whole_sweep differ (potential %d vs %d)\n", sr.t_all, sw.t_all);
            ok = false;
        }
    }
#endif
    if (tf > wh.f.u || tr > wh.r.u) {
        printf("claim W violated: forward %d (bound %d), reverse %d (bound %d)\n", tf, wh.f.u, tr, wh.r.u);
        ok = false;
    }
    if (tf == wh.f.u || tr == wh.r.u) ++cnt->bound_hit;
    // the contract's answer from the two full matrices: a score of 0 is Unmapped, which ranks below every Some
    const int want_strand = tr > tf ? 1 : 0, want_score = want_strand ? tr : tf;
    const int sp = wh.first ? tr : tf;
    const int uo = wh.first ? wh.f.u : wh.r.u;
    if (zsw::seed_strand_settled(sp > 0, sp, uo, wh.first)) {
        ++cnt->settled;
        if (want_strand != wh.first || want_score != sp) {
            printf("claim R violated: settled on strand %d with %d, the two matrices give strand %d with %d (bound of the other strand %d)\n", wh.first, sp,
                   want_strand, want_score, uo);
            ok = false;
        }
    } else {
        ++cnt->both;
    }
    if (!ok) {
        printf("  ref (%d): ", R);
        for (uint8_t x : ref) putchar("ACGTN"[x]);
        printf("\n  read (%d): ", L);
        for (uint8_t x : q) putchar("ACGTN"[x]);
        printf("\n  K %d spacer %d tol %d lambda %d go %d ge %d maxw %d\n", p.K, p.spacer, p.tol, p.lambda, p.go, p.ge, p.maxw);
    }
    return ok;
}

template <class Rnd>
void copy_with_errors(Rnd& rnd, const std::vector<uint8_t>& ref, std::vector<uint8_t>* q, int start, int len, int sub_pm, int indel_pm) {
    const int R = (int)ref.size();
    int i = start;
    while ((int)q->size() < len) {
        uint8_t b = (i >= 0 && i < R) ? ref[i] : (uint8_t)rnd(0, 3);
        const int e = rnd(0, 999);
        if (e < sub_pm) b = (uint8_t)(b < 4 ? (b + rnd(1, 3)) % 4 : rnd(0, 3));  // a different base
        else if (e < sub_pm + indel_pm / 2) { ++i; continue; }
        else if (e < sub_pm + indel_pm) { q->push_back((uint8_t)rnd(0, 3)); continue; }
        q->push_back(b);
        ++i;
    }
    q->resize(len);
}

// One read of the model's classes against `ref`: kind 0-3 a plain copy with few errors, 4 many errors, 5 a chimera of both strands,
// 6 hanging over an end, 7 a long deletion or insertion, 8 one to thirty bases, 9 a chimera of two places, 10-11 random; now and
// then an N or three; half of all reads from the reverse strand.
template <class Rnd>
std::vector<uint8_t> gen_read(Rnd& rnd, const std::vector<uint8_t>& ref, int K, int kind, int L) {
    const int R = (int)ref.size();
    std::vector<uint8_t> q;
    if (kind <= 3) {
        copy_with_errors(rnd, ref, &q, rnd(0, std::max(0, R - L)), L, rnd(0, 30), rnd(0, 10));
    } else if (kind == 4) {
        copy_with_errors(rnd, ref, &q, rnd(0, std::max(0, R - L)), L, rnd(50, 200), rnd(10, 50));
    } else if (kind == 5) {  // a forward piece, then a piece of the reverse strand
        const int l1 = rnd(1, std::max(1, L - 1));
        copy_with_errors(rnd, ref, &q, rnd(0, std::max(0, R - l1)), l1, 10, 0);
        std::vector<uint8_t> t;
        copy_with_errors(rnd, ref, &t, rnd(0, std::max(0, R - L)), L - l1, 10, 0);
        t = revcomp(t);
        q.insert(q.end(), t.begin(), t.end());
    } else if (kind == 6) {
        copy_with_errors(rnd, ref, &q, rnd(0, 1) ? -rnd(1, L / 2 + 1) : R - rnd(1, L / 2 + 1) - L / 2, L, 10, 0);
    } else if (kind == 7) {
        const int l1 = L / 2, st = rnd(0, std::max(0, R - L - 30));
        copy_with_errors(rnd, ref, &q, st, l1, 0, 0);
        int i = st + l1;
        if (rnd(0, 1)) i += rnd(3, 28);
        else
            for (int x = rnd(3, 20); x > 0 && (int)q.size() < L; --x) q.push_back((uint8_t)rnd(0, 3));
        while ((int)q.size() < L) q.push_back(i < R ? ref[i++] : (uint8_t)rnd(0, 3));
    } else if (kind == 8) {
        L = rnd(1, 30);
        if (rnd(0, 1)) copy_with_errors(rnd, ref, &q, rnd(0, std::max(0, R - L)), L, 20, 0);
        else
            for (int i = 0; i < L; ++i) q.push_back((uint8_t)rnd(0, 3));
    } else if (kind == 9) {
        const int l1 = rnd(1, std::max(1, L - 1));
        copy_with_errors(rnd, ref, &q, rnd(0, std::max(0, R - l1)), l1, 10, 0);
        copy_with_errors(rnd, ref, &q, rnd(0, std::max(0, R - L)), L, 10, 0);
    } else {
        for (int i = 0; i < L; ++i) q.push_back((uint8_t)rnd(0, 3));
    }
    (void)K;
    if (rnd(0, 4) == 0)
        for (int x = rnd(1, 3); x > 0; --x) q[rnd(0, (int)q.size() - 1)] = 4;
    if (rnd(0, 1)) q = revcomp(q);
    return q;
}

// Columns between two sampled k-mers without potential, and a reference whose only copy of the read lacks the last column of
// k-mer j, the columns between and the first column of k-mer j + 1: neither k-mer occurs, the path along the copy inserts those
// columns and loses gap_open + 2 * maxw + a gap_extend per column — less than two lambdas where lambda = gap_open.
template <class Rnd>
bool far_only_case(Rnd& rnd, const SeedParams& p, int L, std::vector<uint8_t>* ref, std::vector<uint8_t>* q) {
    int m, stride, c0;
    zsw::seed_layout(L, p.K, p.spacer, &m, &stride, &c0);
    if (m < 2) return false;
    q->resize(L);
    for (auto& x : *q) x = (uint8_t)rnd(0, 3);
    const int j = rnd(0, m - 2);
    const bool all_gaps = rnd(0, 1) == 0;
    for (int i = 0; i + 1 < m; ++i) {
        if (!all_gaps && i != j) continue;
        for (int c = c0 + i * stride + p.K; c < c0 + (i + 1) * stride; ++c) (*q)[c] = 4;
    }
    const int cut_lo = c0 + j * stride + p.K - 1, cut_hi = c0 + (j + 1) * stride + 1;
    ref->clear();
    for (int x = rnd(0, 20); x > 0; --x) ref->push_back((uint8_t)rnd(0, 3));
    for (int c = 0; c < L; ++c)
        if (c < cut_lo || c >= cut_hi) ref->push_back((*q)[c] == 4 ? (uint8_t)rnd(0, 3) : (*q)[c]);
    for (int x = rnd(0, 20); x > 0; --x) ref->push_back((uint8_t)rnd(0, 3));
    if (rnd(0, 1)) *q = revcomp(*q);  // the same on the other strand
    return true;
}

#ifndef ZSW_MODEL_LIB
int report(int n_reads, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const Scheme s = dna(2, -5, 0, 10, 1);
    const int R = 2000, L = 150, K = zsw::seed_k_for(R);
    std::vector<uint8_t> ref(R);
    for (auto& x : ref) x = (uint8_t)rnd(0, 3);
    bool ref_has[32] = {false};
    for (uint8_t x : ref) ref_has[x] = true;
    SeedParams p{};
    if (!zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, ref_has, K, &p)) return 1;
    p.tol = 8;
    std::vector<uint32_t> table((size_t)2 << (2 * K), 0);
    zsw::seed_index_build(p, ref.data(), (uint64_t)R, table.data());
    printf("150-base reads against a random 2 kb reference, half of them from the reverse strand; K = %d, lambda = %d; 2/-5, -10/-1\n", K, p.lambda);
    printf("%-28s %8s %10s %12s\n", "divergence (subst. + indels)", "reads", "settled %", "scored twice");
    const int rates[] = {0, 10, 30, 50, 80, 120, 200, 1000};
    bool ok = true;
    for (int rate : rates) {
        Counters cnt;
        for (int k = 0; k < n_reads && ok; ++k) {
            std::vector<uint8_t> q;
            if (rate == 1000)
                for (int i = 0; i < L; ++i) q.push_back((uint8_t)rnd(0, 3));
            else
                copy_with_errors(rnd, ref, &q, rnd(0, R - L), L, rate, rate / 10);
            if (k & 1) q = revcomp(q);
            ok = check_read(s, p, table, ref, q, 24, &cnt);
        }
        char name[64];
        if (rate == 1000) snprintf(name, sizeof name, "random reads");
        else snprintf(name, sizeof name, "%.1f %% + %.1f %%", rate / 10.0, rate / 100.0);
        printf("%-28s %8ld %10.1f %12ld\n", name, cnt.reads, 100.0 * cnt.settled / std::max(1l, cnt.reads), cnt.both);
    }
    return ok ? 0 : 1;
}

int run_checks(int iters, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const Scheme schemes[] = {dna(2, -5, 0, 10, 1), dna(1, -1, 0, 2, 1), dna(3, -2, 0, 5, 0), dna(1, -3, 0, 5, 2), dna(5, -4, 0, 8, 0),
                              dna(2, -5, -1, 10, 1), dna(4, -6, 1, 12, 2), dna(2, -2, 0, 3, 3),
                              // mismatch loss >= gap_open: lambda = gap_open, an insertion run is the cheapest way through a k-mer
                              dna(2, -10, 0, 10, 1), dna(2, -5, 0, 5, 1), dna(3, -9, 0, 6, 1), dna(2, -10, 0, 10, 0)};
    Counters cnt, plain;
    long structured = 0;
    bool all_ok = true;
    for (int it = 0; it < iters && all_ok; ++it) {
        const Scheme& s = schemes[it % (sizeof(schemes) / sizeof(schemes[0]))];
        const int R = rnd(60, 420);
        std::vector<uint8_t> ref(R);
        for (auto& x : ref) x = (uint8_t)rnd(0, 3);
        if (rnd(0, 2) == 0 && R > 120) {  // an inverted repeat: the reverse complement of a segment, elsewhere
            const int len = rnd(20, 50), from = rnd(0, R - len), to = rnd(0, R - len);
            std::vector<uint8_t> seg(ref.begin() + from, ref.begin() + from + len);
            seg = revcomp(seg);
            for (int i = 0; i < len; ++i) ref[to + i] = seg[i];
        }
        if (rnd(0, 3) == 0 && R > 100) {  // a palindrome: a segment followed by its own reverse complement
            const int len = rnd(6, 25), at = rnd(0, R - 2 * len);
            for (int i = 0; i < len; ++i) ref[at + 2 * len - 1 - i] = COMP5[ref[at + i]];
        }
        if (rnd(0, 3) == 0 && R > 100) {  // tandem repeat (AT repeats are their own reverse complement)
            const int unit = rnd(1, 6), len = rnd(20, 60), at = rnd(0, R - len);
            for (int i = unit; i < len; ++i) ref[at + i] = ref[at + i - unit];
        }
        if (rnd(0, 1) == 0)  // N runs of one to five
            for (int k = rnd(1, 5); k > 0; --k) {
                const int len = rnd(1, 5), at = rnd(0, R - len);
                for (int i = 0; i < len; ++i) ref[at + i] = 4;
            }
        bool ref_has[32] = {false};
        for (uint8_t x : ref) ref_has[x] = true;
        SeedParams p{};
        const int K = rnd(3, 6);
        if (!zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, ref_has, K, &p)) continue;
        if (rnd(0, 2) == 0) p.spacer += rnd(0, 6);  // sparser sampling is valid too
        p.tol = rnd(0, 8);
        const int min_len = rnd(0, 1) ? 0 : rnd(K, 24);
        std::vector<uint32_t> table((size_t)2 << (2 * K), 0);
        zsw::seed_index_build(p, ref.data(), (uint64_t)R, table.data());
        for (int k = 0; k < 60 && all_ok; ++k) {
            const int kind = rnd(0, 11);
            const std::vector<uint8_t> q = gen_read(rnd, ref, K, kind, rnd(K, std::min(R, 90)));
            const bool is_plain = kind <= 3;
            all_ok = check_read(s, p, table, ref, q, min_len, is_plain ? &plain : &cnt);
        }
        for (int k = 0; k < 24 && all_ok; ++k) {
            std::vector<uint8_t> aref, aq;
            SeedParams pa{};
            bool has[32] = {false};
            has[0] = has[1] = has[2] = has[3] = true;
            if (!zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, has, K, &pa)) break;
            pa.tol = p.tol;
            if (rnd(0, 3) == 0) pa.spacer += rnd(0, 3);
            if (!far_only_case(rnd, pa, rnd(2 * (K + pa.spacer), 96), &aref, &aq)) continue;
            std::vector<uint32_t> atable((size_t)2 << (2 * K), 0);
            zsw::seed_index_build(pa, aref.data(), (uint64_t)aref.size(), atable.data());
            all_ok = check_read(s, pa, atable, aref, aq, 0, &cnt);
            ++structured;
        }
    }
    printf("reads %ld (settled %ld, scored twice %ld, bound reached %ld); plain reads %ld (settled %ld); structured cases %ld\n", cnt.reads + plain.reads,
           cnt.settled + plain.settled, cnt.both + plain.both, cnt.bound_hit + plain.bound_hit, plain.reads, plain.settled, structured);
    if (!all_ok) return 1;
    if (plain.reads > 200 && plain.settled * 4 < plain.reads) {
        printf("the checks are vacuous: fewer than a quarter of the plain reads are settled\n");
        return 1;
    }
    printf("strand_bound OK\n");
    return 0;
}
#endif

}  // namespace

#ifdef ZSW_MODEL_LIB
// What strand_seed_kernel stores for each of n reads (residue indices q[offsets[i] .. offsets[i + 1])): out[5 * i ..] = support of
// the anchor vote forward / reverse, claim W's bound forward / reverse as 16-bit values (-1: none), the strand that runs first.
// comp: residue index -> residue index of the complement. Returns -1 if the matrix allows no index (the kernel then has no bounds).
extern "C" int zsw_model_strand_batch(const int32_t* w, int S, int go, int ge, const uint8_t* ref, int R, const uint8_t* q, const int64_t* offsets, int n,
                                      int K, int tol, int min_len, const uint8_t* comp, int32_t* out) {
    bool ref_has[32] = {false};
    for (int i = 0; i < R; ++i) ref_has[ref[i] & 31] = true;
    SeedParams p{};
    if (!zsw::seed_analyze(S, w, go, ge, ref_has, K, &p)) return -1;
    p.tol = tol;
    std::vector<uint32_t> table((size_t)2 << (2 * K), 0);
    zsw::seed_index_build(p, ref, (uint64_t)R, table.data());
    for (int i = 0; i < n; ++i) {
        const Whole wh = whole_of(p, table, q + offsets[i], (int)(offsets[i + 1] - offsets[i]), comp, min_len);
        const uint32_t uf = zsw::seed_bound_u16(wh.f.u), ur = zsw::seed_bound_u16(wh.r.u);
        out[5 * i] = wh.f.support;
        out[5 * i + 1] = wh.r.support;
        out[5 * i + 2] = uf == 0xffffu ? -1 : (int32_t)uf;
        out[5 * i + 3] = ur == 0xffffu ? -1 : (int32_t)ur;
        out[5 * i + 4] = wh.first;
    }
    return 0;
}

// n reads of the model's classes (gen_read) against `ref` (residue indices), lengths of up to max_len: residue indices into q
// (capacity cap), offsets[n + 1]. Returns the number of reads written (fewer than n if q is full).
extern "C" int zsw_model_strand_reads(uint64_t seed, const uint8_t* ref, int R, int n, int K, int max_len, uint8_t* q, int64_t cap, int64_t* offsets) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const std::vector<uint8_t> r(ref, ref + R);
    offsets[0] = 0;
    int i = 0;
    for (; i < n; ++i) {
        const std::vector<uint8_t> read = gen_read(rnd, r, K, rnd(0, 11), rnd(K, std::min(R, max_len)));
        if (offsets[i] + (int64_t)read.size() > cap) break;
        memcpy(q + offsets[i], read.data(), read.size());
        offsets[i + 1] = offsets[i] + (int64_t)read.size();
    }
    return i;
}

extern "C" int zsw_model_strand_settled(int some_p, long long s_p, long long u_o, int p) { return zsw::seed_strand_settled(some_p != 0, s_p, u_o, p) ? 1 : 0; }
#else
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "report")) return report(argc > 2 ? atoi(argv[2]) : 2000, argc > 3 ? strtoull(argv[3], nullptr, 10) : 1);
    return run_checks(argc > 1 ? atoi(argv[1]) : 50, argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
}
#endif
