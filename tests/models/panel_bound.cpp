// panel_bound.cpp — host model of the panel score pass (zoe_amd/csrc/zsw_panel.hip). It compiles the header the kernels use
// (zsw_seed.hpp: seed_whole_bound, seed_panel_ruled_out, seed_panel_todo) and checks, with plain integers against the full Gotoh
// matrix of the read against EVERY member:
//   W  no local alignment of the read against member k scores more than seed_whole_bound().u under that member's parameters and
//      index — for every member;
//   P  the decision rule: the member with the largest support of the anchor vote runs first (ties: the lowest); whenever
//      seed_panel_ruled_out lets a member go unscored, the answer of the contract (the member that ranks highest — OVERFLOWED >
//      SOME by score > UNMAPPED —, ties to the lowest member, by all the full matrices) is the answer over the members that are
//      scored, merged by the same ranking.
// Panels of 2 to 6 members: a near copy of another member, members identical to another, members with N runs, each member with
// its own K — small ones (3 to 6) over members of 60 to 420 bases, so that chance occurrences are common, and every eighth panel the
// K the library picks (seed_k_for) for members on both sides of 2,048 bases. Reads: exact copies and copies of each member with
// substitutions, indels and N, chimeras of two members, random reads, reads of 1 to 30 bases. A quarter of the panels run with an
// overflow threshold low enough that many reads are OVERFLOWED against several members.
// usage: panel_bound <iterations> <seed>            the checks
//        panel_bound report <reads> <seed>          per divergence rate: the share of 150-base reads settled after one score and the
//                                                   mean number of members scored per read (2/-5, -10/-1; two panels of 8)
// -DZSW_MODEL_LIB: no main; zsw_model_panel_batch() returns what the kernel stores per read (tests/test_gpu_panel.py).
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

struct Member {
    std::vector<uint8_t> ref;
    bool usable = false;
    SeedParams p{};
    std::vector<uint32_t> table;
};

// the member's parameters and index as seed_index_update builds them (K: the k-mer length; tol: the anchor vote's tolerance)
void index_member(const Scheme& s, Member* m, int K, int tol, int extra_spacer = 0) {
    bool ref_has[32] = {false};
    for (uint8_t x : m->ref) ref_has[x & 31] = true;
    m->p = SeedParams{};
    m->usable = s.S <= 7 && zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, ref_has, K, &m->p);
    if (!m->usable) return;
    m->p.spacer += extra_spacer;
    m->p.tol = tol;
    m->table.assign((size_t)2 << (2 * K), 0);
    zsw::seed_index_build(m->p, m->ref.data(), (uint64_t)m->ref.size(), m->table.data());
}

// what the panel pass derives from one read before anything is scored: per member the support and the 16-bit bound, the first choice
struct Seeded {
    int first = 0;
    std::vector<int> support;
    std::vector<uint16_t> u16;
};

Seeded seed_of(const std::vector<Member>& panel, const uint8_t* q, int L, int min_len) {
    Seeded o;
    int best = 0;
    for (size_t k = 0; k < panel.size(); ++k) {
        const Member& m = panel[k];
        int support = 0;
        uint32_t u = 0xffffu;
        if (m.usable) {
            const zsw::SeedWhole wh = zsw::seed_whole_bound(
                m.p, L, min_len, [&](int c) { return zsw::seed_cell(m.p, (int)q[c]); },
                [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
                    *f1 = m.table[2 * (size_t)code];
                    *l1 = m.table[2 * (size_t)code + 1];
                });
            support = wh.support;
            u = zsw::seed_bound_u16(wh.u);
        }
        o.support.push_back(support);
        o.u16.push_back((uint16_t)u);
        if (support > best) {
            best = support;
            o.first = (int)k;
        }
    }
    return o;
}

// OVERFLOWED > SOME by score > UNMAPPED, as the merge kernel ranks
long long rank_of(int score, int thr) { return score >= thr ? 2ll << 32 : score > 0 ? (1ll << 32) | score : 0; }

struct Counters {
    long reads = 0, settled = 0, scored = 0, bound_hit = 0, ties = 0, overflowed = 0;
};

template <class Rnd>
void copy_with_errors(Rnd& rnd, const std::vector<uint8_t>& ref, std::vector<uint8_t>* q, int start, int len, int sub_pm, int indel_pm) {
    const int R = (int)ref.size();
    const size_t want = q->size() + (size_t)len;
    int i = start;
    while (q->size() < want) {
        uint8_t b = (i >= 0 && i < R) ? ref[i] : (uint8_t)rnd(0, 3);
        const int e = rnd(0, 999);
        if (e < sub_pm) b = (uint8_t)(b < 4 ? (b + rnd(1, 3)) % 4 : rnd(0, 3));  // a different base
        else if (e < sub_pm + indel_pm / 2) { ++i; continue; }
        else if (e < sub_pm + indel_pm) { q->push_back((uint8_t)rnd(0, 3)); continue; }
        q->push_back(b);
        ++i;
    }
}

bool check_read(const Scheme& s, const std::vector<Member>& panel, const std::vector<uint8_t>& q, int min_len, int thr, Counters* cnt) {
    const int K = (int)panel.size(), L = (int)q.size();
    const Seeded sd = seed_of(panel, q.data(), L, min_len);
    std::vector<int> t(K);
    bool ok = true;
    for (int k = 0; k < K; ++k) {
        t[k] = gotoh(s.w.data(), s.S, s.go, s.ge, panel[k].ref.data(), (int)panel[k].ref.size(), q.data(), L);
        if (sd.u16[k] != 0xffffu && t[k] > (int)sd.u16[k]) {
            printf("claim W violated: member %d scores %d, its bound is %d\n", k, t[k], (int)sd.u16[k]);
            ok = false;
        }
        if (sd.u16[k] != 0xffffu && t[k] == (int)sd.u16[k]) ++cnt->bound_hit;
    }
    ++cnt->reads;
    // the contract's answer from all the full matrices
    int want = 0;
    for (int k = 1; k < K; ++k)
        if (rank_of(t[k], thr) > rank_of(t[want], thr)) want = k;
    int n_best = 0;
    for (int k = 0; k < K; ++k) n_best += rank_of(t[k], thr) == rank_of(t[want], thr) && t[want] > 0;
    if (n_best > 1) ++cnt->ties;
    if (t[want] >= thr) ++cnt->overflowed;
    // the pass: the first choice is scored, the rule lists the others, the merge keeps the highest rank from the lowest member
    const int p = sd.first;
    const bool some_p = t[p] > 0 && t[p] < thr;
    const unsigned long long todo = zsw::seed_panel_todo(K, p, some_p, (long long)t[p], sd.u16.data());
    int got = p;
    for (int k = 0; k < K; ++k) {
        if (!((todo >> k) & 1ull)) continue;
        const long long mine = rank_of(t[k], thr), held = rank_of(t[got], thr);
        if (mine > held || (mine == held && k < got)) got = k;
    }
    if (todo == 0) ++cnt->settled;
    cnt->scored += 1 + __builtin_popcountll(todo);
    if ((todo >> p) & 1ull) {
        printf("the first choice %d is listed again\n", p);
        ok = false;
    }
    if (got != want || t[got] != t[want]) {
        printf("claim P violated: the pass answers member %d with %d, the full matrices give member %d with %d (first choice %d, threshold %d)\n", got, t[got],
               want, t[want], p, thr);
        ok = false;
    }
    if (!ok) {
        for (int k = 0; k < K; ++k)
            printf("  member %d: %d bases, K %d, lambda %d, support %d, bound %d, score %d%s\n", k, (int)panel[k].ref.size(), panel[k].p.K, panel[k].p.lambda,
                   sd.support[k], sd.u16[k] == 0xffffu ? -1 : (int)sd.u16[k], t[k], ((todo >> k) & 1ull) ? ", listed" : "");
        printf("  read (%d): ", L);
        for (uint8_t x : q) putchar("ACGTN"[x]);
        printf("\n");
    }
    return ok;
}

template <class Rnd>
std::vector<uint8_t> random_seq(Rnd& rnd, int len) {
    std::vector<uint8_t> r(len);
    for (auto& x : r) x = (uint8_t)rnd(0, 3);
    return r;
}

// A panel: member 0 random, every further one random, a near copy of an earlier one (1 to 5 % substitutions, now and then an
// indel), identical to an earlier one, or random with N runs of one to five. len_of(fresh): the length of the fresh-th random member.
template <class Rnd, class Len>
std::vector<Member> make_panel(Rnd& rnd, int n, Len len_of, bool second_fresh) {
    std::vector<Member> panel(n);
    int fresh = 0;
    for (int k = 0; k < n; ++k) {
        const int kind = k == 0 || (k == 1 && second_fresh) ? 0 : rnd(0, 3);
        if (kind == 1) {
            const std::vector<uint8_t>& from = panel[rnd(0, k - 1)].ref;
            copy_with_errors(rnd, from, &panel[k].ref, 0, (int)from.size(), rnd(10, 50), rnd(0, 4));
        } else if (kind == 2) {
            panel[k].ref = panel[rnd(0, k - 1)].ref;
        } else {
            panel[k].ref = random_seq(rnd, len_of(fresh++));
            if (kind == 3)
                for (int r = rnd(1, 5); r > 0; --r) {
                    const int len = rnd(1, 5), at = rnd(0, (int)panel[k].ref.size() - len);
                    for (int i = 0; i < len; ++i) panel[k].ref[at + i] = 4;
                }
        }
    }
    return panel;
}

// One read of the model's classes: kind 0 an exact copy of a piece of a member, 1-3 a copy with few errors, 4 many errors, 5-6 a
// chimera of two members, 7 one to thirty bases, 8-9 random; now and then an N or three.
template <class Rnd>
std::vector<uint8_t> gen_read(Rnd& rnd, const std::vector<Member>& panel, int kind, int L) {
    const int n = (int)panel.size();
    const std::vector<uint8_t>& a = panel[rnd(0, n - 1)].ref;
    const std::vector<uint8_t>& b = panel[rnd(0, n - 1)].ref;
    L = std::min<int>(L, (int)std::min(a.size(), b.size()));
    std::vector<uint8_t> q;
    if (kind == 0) {
        const int at = rnd(0, (int)a.size() - L);
        q.assign(a.begin() + at, a.begin() + at + L);
        return q;
    } else if (kind <= 3) {
        copy_with_errors(rnd, a, &q, rnd(0, (int)a.size() - L), L, rnd(0, 30), rnd(0, 10));
    } else if (kind == 4) {
        copy_with_errors(rnd, a, &q, rnd(0, (int)a.size() - L), L, rnd(50, 200), rnd(10, 50));
    } else if (kind <= 6) {
        const int l1 = rnd(1, std::max(1, L - 1));
        copy_with_errors(rnd, a, &q, rnd(0, (int)a.size() - l1), l1, 10, 0);
        if (L > l1) copy_with_errors(rnd, b, &q, rnd(0, (int)b.size() - (L - l1)), L - l1, 10, 0);
    } else if (kind == 7) {
        L = rnd(1, std::min(30, L));
        if (rnd(0, 1)) copy_with_errors(rnd, a, &q, rnd(0, (int)a.size() - L), L, 20, 0);
        else q = random_seq(rnd, L);
    } else {
        q = random_seq(rnd, L);
    }
    if (rnd(0, 4) == 0)
        for (int x = rnd(1, 3); x > 0; --x) q[rnd(0, (int)q.size() - 1)] = 4;
    return q;
}

#ifndef ZSW_MODEL_LIB
int report(int n_reads, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const Scheme s = dna(2, -5, 0, 10, 1);
    const int L = 150, NM = 8;
    for (int variant = 0; variant < 2; ++variant) {
        std::vector<Member> panel(NM);
        for (int k = 0; k < NM; ++k) {
            if (variant == 1 && (k & 1)) copy_with_errors(rnd, panel[k - 1].ref, &panel[k].ref, 0, (int)panel[k - 1].ref.size(), 100, 10);
            else panel[k].ref = random_seq(rnd, rnd(900, 2400));
            index_member(s, &panel[k], zsw::seed_k_for(panel[k].ref.size()), 8);
            if (!panel[k].usable) return 1;
        }
        printf("%s; 150-base reads drawn evenly from the members; 2/-5, -10/-1\n",
               variant == 0 ? "panel of 8 unrelated random members of 900 to 2,400 bases" : "panel of 4 pairs of members 10 % + 1 % apart, 900 to 2,400 bases");
        printf("%-28s %8s %10s %16s\n", "divergence (subst. + indels)", "reads", "settled %", "members per read");
        const int rates[] = {0, 10, 30, 50, 80, 120, 200, 1000};
        for (int rate : rates) {
            Counters cnt;
            for (int i = 0; i < n_reads; ++i) {
                const Member& from = panel[i % NM];
                std::vector<uint8_t> q;
                if (rate == 1000) q = random_seq(rnd, L);
                else copy_with_errors(rnd, from.ref, &q, rnd(0, (int)from.ref.size() - L), L, rate, rate / 10);
                const Seeded sd = seed_of(panel, q.data(), L, 24);
                const Member& p = panel[sd.first];
                const int tp = gotoh(s.w.data(), s.S, s.go, s.ge, p.ref.data(), (int)p.ref.size(), q.data(), L);
                const unsigned long long todo = zsw::seed_panel_todo(NM, sd.first, tp > 0, (long long)tp, sd.u16.data());
                ++cnt.reads;
                cnt.settled += todo == 0;
                cnt.scored += 1 + __builtin_popcountll(todo);
            }
            char name[64];
            if (rate == 1000) snprintf(name, sizeof name, "random reads");
            else snprintf(name, sizeof name, "%.1f %% + %.1f %%", rate / 10.0, rate / 100.0);
            printf("%-28s %8ld %10.1f %16.2f\n", name, cnt.reads, 100.0 * cnt.settled / std::max(1l, cnt.reads), (double)cnt.scored / std::max(1l, cnt.reads));
        }
    }
    return 0;
}

int run_checks(int iters, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const Scheme schemes[] = {dna(2, -5, 0, 10, 1), dna(1, -1, 0, 2, 1), dna(3, -2, 0, 5, 0), dna(1, -3, 0, 5, 2), dna(5, -4, 0, 8, 0),
                              dna(2, -5, -1, 10, 1), dna(4, -6, 1, 12, 2), dna(2, -2, 0, 3, 3),
                              // mismatch loss >= gap_open: lambda = gap_open, an insertion run is the cheapest way through a k-mer
                              dna(2, -10, 0, 10, 1), dna(2, -5, 0, 5, 1), dna(3, -9, 0, 6, 1), dna(2, -10, 0, 10, 0)};
    const int n_schemes = (int)(sizeof(schemes) / sizeof(schemes[0]));
    Counters cnt;
    long panels = 0, k8 = 0, k9 = 0;
    bool all_ok = true;
    for (int it = 0; it < iters && all_ok; ++it) {
        // every eighth panel as the library indexes it; the scheme advances once per round of eight, so both kinds meet every scheme
        const bool library_k = it % 8 == 7;
        const Scheme& s = schemes[(it + it / 8) % n_schemes];
        const int n = rnd(2, 6);
        std::vector<Member> panel =
            library_k ? make_panel(rnd, n, [&](int fresh) { return fresh == 0 ? rnd(1900, 2048) : fresh == 1 ? rnd(2049, 2300) : rnd(200, 600); }, true)
                      : make_panel(rnd, n, [&](int) { return rnd(60, 420); }, false);
        const int tol = rnd(0, 8);
        bool usable = true;
        for (Member& m : panel) {
            const int K = library_k ? zsw::seed_k_for(m.ref.size()) : rnd(3, 6);
            index_member(s, &m, K, library_k ? 8 : tol, !library_k && rnd(0, 2) == 0 ? rnd(0, 6) : 0);
            usable = usable && m.usable;
            k8 += library_k && K == 8;
            k9 += library_k && K == 9;
        }
        if (!usable) continue;
        ++panels;
        const int min_len = library_k ? 24 : rnd(0, 1) ? 0 : rnd(6, 24);
        const int thr = it % 4 == 1 ? rnd(20, 120) : 1 << 30;
        const int n_reads = library_k ? 16 : 40;
        for (int k = 0; k < n_reads && all_ok; ++k) {
            const std::vector<uint8_t> q = gen_read(rnd, panel, rnd(0, 9), library_k ? rnd(60, 150) : rnd(6, 90));
            all_ok = check_read(s, panel, q, min_len, thr, &cnt);
        }
    }
    printf("panels %ld (members indexed with K = 8: %ld, K = 9: %ld); reads %ld (settled after one score %ld, members scored %ld, bound reached %ld, ties %ld, "
           "overflowed %ld)\n", panels, k8, k9, cnt.reads, cnt.settled, cnt.scored, cnt.bound_hit, cnt.ties, cnt.overflowed);
    if (!all_ok) return 1;
    if (cnt.reads > 2000 && (cnt.settled * 10 < cnt.reads || cnt.ties * 50 < cnt.reads || cnt.overflowed * 50 < cnt.reads || (iters >= 16 && (!k8 || !k9)))) {
        printf("the checks are vacuous: too few reads are settled, tie or overflow, or a K of the library did not occur\n");
        return 1;
    }
    printf("panel_bound OK\n");
    return 0;
}
#endif

}  // namespace

#ifdef ZSW_MODEL_LIB
// What panel_seed_kernel stores for each of n reads (residue indices q[offsets[i] .. offsets[i + 1])) against the n_refs members
// refs[ref_offsets[k] .. ref_offsets[k + 1]) (residue indices), indexed as seed_index_update does: out[(2 + 2 * n_refs) * i ..] = the
// first choice, 0, the n_refs supports, the n_refs bounds as 16-bit values (-1: none). Returns the number of members with an index.
extern "C" int zsw_model_panel_batch(const int32_t* w, int S, int go, int ge, const uint8_t* refs, const int64_t* ref_offsets, int n_refs, const uint8_t* q,
                                     const int64_t* offsets, int n, int tol, int min_len, int32_t* out) {
    Scheme s;
    s.S = S;
    s.w.assign(w, w + S * S);
    s.go = go;
    s.ge = ge;
    std::vector<Member> panel(n_refs);
    int usable = 0;
    for (int k = 0; k < n_refs; ++k) {
        panel[k].ref.assign(refs + ref_offsets[k], refs + ref_offsets[k + 1]);
        index_member(s, &panel[k], zsw::seed_k_for(panel[k].ref.size()), tol);
        usable += panel[k].usable;
    }
    const size_t ints = 2 + 2 * (size_t)n_refs;
    for (int i = 0; i < n; ++i) {
        int32_t* r = out + ints * i;
        if (!usable) {  // the kernel does not run: member 0 first, no bounds
            r[0] = r[1] = 0;
            for (int k = 0; k < n_refs; ++k) r[2 + k] = 0, r[2 + n_refs + k] = -1;
            continue;
        }
        const Seeded sd = seed_of(panel, q + offsets[i], (int)(offsets[i + 1] - offsets[i]), min_len);
        r[0] = sd.first;
        r[1] = 0;
        for (int k = 0; k < n_refs; ++k) {
            r[2 + k] = sd.support[k];
            r[2 + n_refs + k] = sd.u16[k] == 0xffffu ? -1 : (int32_t)sd.u16[k];
        }
    }
    return usable;
}

// the members still to score once the first choice p has (some_p, s_p: its status is SOME, its score); bounds: -1 = none
extern "C" unsigned long long zsw_model_panel_todo(int n_refs, int p, int some_p, long long s_p, const int32_t* bounds) {
    uint16_t u16[64];
    for (int k = 0; k < n_refs && k < 64; ++k) u16[k] = bounds[k] < 0 ? (uint16_t)0xffffu : (uint16_t)bounds[k];
    return zsw::seed_panel_todo(n_refs, p, some_p != 0, s_p, u16);
}
#else
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "report")) return report(argc > 2 ? atoi(argv[2]) : 500, argc > 3 ? strtoull(argv[3], nullptr, 10) : 1);
    return run_checks(argc > 1 ? atoi(argv[1]) : 48, argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
}
#endif
