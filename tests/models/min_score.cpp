// min_score.cpp — host model of ZSW_OPTION_MIN_SCORE (include/zoe_sw.h): a read is settled as "below the caller's minimum T" by an
// upper bound of its score where the seeded pass has one, and by its exact score otherwise. It compiles the header the kernels use
// (zsw_seed.hpp: seed_read<true>'s u_whole, seed_band_upper, seed_below_min) and, through their ZSW_MODEL_LIB mode, the models that
// hold the two claims the bounds are derived from — strand_bound.cpp (claim W and its reads) and seed_band.cpp (the band walk: every
// band cell >= its true H, every outside cell <= oa / ob) — and checks with plain integers against the full Gotoh matrix:
//   W   the bound seed_read<true> returns equals seed_whole_bound().u (same sweep, same entries) and is >= the matrix's maximum;
//       a read shorter than min_len gets the potential of its columns either way;
//   B   for every read the band walks, accepted or not, in score-only and ends tagging: through seed_band_upper every band cell
//       bounds its true H, oa / ob bound every cell above / below the band, and the whole is >= the matrix's maximum;
//   D   the decision: for T in {1, true, true + 1, bound, bound + 1, thr, thr + 1} the contract's answer computed from the full
//       matrix (OVERFLOWED from thr on; BELOW if 0 or below min(T, thr); else SOME with the score) equals "BELOW if
//       seed_below_min(bound, min(T, thr)), else the exact score's answer" — for the whole-read bound and both band bounds.
// usage: min_score <iterations> <seed>        the checks
//        min_score report <reads> <seed>      150-base reads vs 2 kb, 2/-5, -10/-1, K = 8: per divergence rate and T, the share of
//                                             reads below T and which route settles them
// -DZSW_MIN_SCORE_LIB: no main; zsw_model_min_whole() and the two functions of the decision for tests/test_gpu_min_score.py (with
// zsw_model_band() of seed_band.cpp, which this file includes).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zoe_amd/csrc/zsw_seed.hpp"

#ifndef ZSW_MODEL_LIB
#define ZSW_MODEL_LIB
#endif
namespace strand_model {
#include "strand_bound.cpp"
}
namespace band_model {
#include "seed_band.cpp"
}

namespace {

using zsw::SeedParams;
using band_model::Geometry;
using band_model::Scheme;
using band_model::dna;

enum { ST_SOME = 0, ST_OVERFLOWED = 1, ST_BELOW = 4 };

struct Answer {
    int status;
    long long score;
    bool operator==(const Answer& o) const { return status == o.status && score == o.score; }
};

// the contract of include/zoe_sw.h from the true score (T > 0)
Answer contract(long long truth, long long T, long long thr) {
    if (truth >= thr) return {ST_OVERFLOWED, 0};
    if (truth == 0 || truth < std::min(T, thr)) return {ST_BELOW, 0};
    return {ST_SOME, truth};
}
// what the library does: the bound where it settles the read, the exact score otherwise
Answer routed(long long bound, long long truth, long long T, long long thr) {
    if (zsw::seed_below_min(bound, std::min(T, thr))) return {ST_BELOW, 0};
    return contract(truth, T, thr);
}

bool check_decision(const char* what, long long bound, long long truth, long long thr) {
    const long long Ts[] = {1, truth, truth + 1, bound, bound + 1, thr, thr + 1};
    for (long long T : Ts) {
        if (T < 1) continue;
        const Answer want = contract(truth, T, thr), got = routed(bound, truth, T, thr);
        if (!(want == got)) {
            printf("decision rule violated (%s): true %lld, bound %lld, T %lld, thr %lld: the matrix says (%d, %lld), the routes (%d, %lld)\n", what, truth, bound, T, thr,
                   want.status, want.score, got.status, got.score);
            return false;
        }
    }
    return true;
}

struct Counters {
    long reads = 0, anchored = 0, walks = 0, unaccepted = 0, whole_tight = 0, band_tight = 0;
};

void dump(const SeedParams& p, const std::vector<uint8_t>& ref, const std::vector<uint8_t>& q) {
    printf("  ref (%d): ", (int)ref.size());
    for (uint8_t x : ref) putchar("ACGTN"[x]);
    printf("\n  read (%d): ", (int)q.size());
    for (uint8_t x : q) putchar("ACGTN"[x]);
    printf("\n  K %d spacer %d Dn %d Dm %d tol %d lambda %d go %d ge %d maxw %d\n", p.K, p.spacer, p.Dn, p.Dm, p.tol, p.lambda, p.go, p.ge, p.maxw);
}

// W, B and D for one read. walk: the scheme is one of seed_band.cpp's. g.dtmin / g.dtmax are offsets from the read's anchor.
bool check_read(const Scheme& s, const SeedParams& p, const std::vector<uint32_t>& table, const std::vector<uint8_t>& ref, const std::vector<uint8_t>& q, int min_len,
                bool walk, Geometry g, long long thr, int thr_delta, Counters* cnt) {
    const int R = (int)ref.size(), L = (int)q.size();
    auto cell = [&](int c) { return zsw::seed_cell(p, (int)q[c]); };
    auto look = [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
        *f1 = table[2 * (size_t)code];
        *l1 = table[2 * (size_t)code + 1];
    };
    ++cnt->reads;
    const band_model::Truth t = band_model::gotoh_full(s, ref, q);
    if (thr == 0) thr = std::max(1, t.best + thr_delta);  // a threshold next to the read's own score
    const zsw::SeedRead sr = zsw::seed_read<true>(p, L, cell, look);
    bool ok = true;
    // W: the sweep of seed_read against claim W's own; a read the kernel does not sweep gets the potential of its columns
    const int whole = L < min_len ? sr.t_all : sr.u_whole;
    const zsw::SeedWhole w0 = zsw::seed_whole_bound(p, L, 0, cell, look), wm = zsw::seed_whole_bound(p, L, min_len, cell, look);
    if (sr.u_whole != w0.u || whole != wm.u || sr.t_all != w0.t_all) {
        printf("whole-read bound: seed_read returns %d (potential %d), seed_whole_bound %d (potential %d); with min_len %d: %d vs %d\n", sr.u_whole, sr.t_all, w0.u,
               w0.t_all, min_len, whole, wm.u);
        ok = false;
    }
    if (t.best > whole) {
        printf("claim W violated: the matrix holds %d, the whole-read bound is %d\n", t.best, whole);
        ok = false;
    }
    if (t.best == whole) ++cnt->whole_tight;
    if (ok) ok = check_decision("whole-read bound", whole, t.best, thr);
    if (ok && walk && sr.ok) {
        ++cnt->anchored;
        g.dtmin += sr.dt;
        g.dtmax += sr.dt;
        g.R = R;
        const int C = g.C;
        for (int tag = -1; tag <= 1 && ok; tag += 2) {
            const band_model::Walk w = band_model::walk_band(s, p, sr, ref, q, g, tag, true);
            ++cnt->walks;
            const int upper = zsw::seed_band_upper(w.best2, w.oa, w.ob);
            for (int k = 0; k < g.n_strips && ok; ++k) {
                const int top = g.top(k), bot = g.bot(k);
                for (int c = k * C; c < std::min(L, (k + 1) * C) && ok; ++c)
                    for (int r = 0; r < R && ok; ++r) {
                        const int h = t.H[(size_t)r * L + c];
                        const bool in = r >= top && r < bot;
                        const int b = in ? zsw::seed_band_upper(w.U[(size_t)r * L + c], 0, 0) : r < top ? zsw::seed_band_upper(0, w.oa, 0) : zsw::seed_band_upper(0, 0, w.ob);
                        if (in && w.U[(size_t)r * L + c] == 0xffffffffu) {
                            printf("band bound: cell (%d,%d) of the band was not walked\n", r, c);
                            ok = false;
                        } else if (h > b) {
                            printf("band bound violated: cell (%d,%d) %s the band holds %d, seed_band_upper gives %d (tag %d, value %u, oa %d, ob %d)\n", r, c,
                                   in ? "of" : r < top ? "above" : "below", h, b, tag, in ? w.U[(size_t)r * L + c] : 0u, w.oa, w.ob);
                            ok = false;
                        }
                    }
            }
            if (ok && t.best > upper) {
                printf("band bound violated: the matrix holds %d, seed_band_upper(%u, %d, %d) = %d (tag %d)\n", t.best, w.best2, w.oa, w.ob, upper, tag);
                ok = false;
            }
            const int S = (int)(w.best2 >> 1), outside = std::max(w.oa, w.ob);
            const bool accepted = !(w.best2 & 1u) && (tag < 0 ? outside <= S : outside < S);
            if (!accepted) ++cnt->unaccepted;
            if (t.best == upper) ++cnt->band_tight;
            if (ok) ok = check_decision(tag < 0 ? "band bound, score-only tag" : "band bound, ends tag", upper, t.best, thr);
        }
    }
    if (!ok) dump(p, ref, q);
    return ok;
}

int run_checks(int iters, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    // strand_bound.cpp's twelve schemes; the first eleven are seed_band.cpp's (the band's doubled domain wants gap_extend > 0 or a
    // mismatch the tables hold: its own list), so the last one takes the whole-read checks only
    const Scheme schemes[] = {dna(2, -5, 0, 10, 1), dna(1, -1, 0, 2, 1), dna(3, -2, 0, 5, 0), dna(1, -3, 0, 5, 2), dna(5, -4, 0, 8, 0), dna(2, -5, -1, 10, 1),
                              dna(4, -6, 1, 12, 2), dna(2, -2, 0, 3, 3), dna(2, -10, 0, 10, 1), dna(2, -5, 0, 5, 1), dna(3, -9, 0, 6, 1), dna(2, -10, 0, 10, 0)};
    const int n_schemes = (int)(sizeof(schemes) / sizeof(schemes[0]));
    Counters cnt;
    long structured = 0;
    bool all_ok = true;
    for (int it = 0; it < iters && all_ok; ++it) {
        const int si = it % n_schemes;
        const Scheme& s = schemes[si];
        const int R = rnd(60, 420);
        std::vector<uint8_t> ref(R);
        for (auto& x : ref) x = (uint8_t)rnd(0, 3);
        if (rnd(0, 2) == 0 && R > 120) {  // a repeat
            const int len = rnd(20, 50), from = rnd(0, R - len), to = rnd(0, R - len);
            for (int i = 0; i < len; ++i) ref[to + i] = ref[from + i];
        }
        if (rnd(0, 3) == 0 && R > 100) {  // a tandem repeat
            const int unit = rnd(1, 6), len = rnd(20, 60), at = rnd(0, R - len);
            for (int i = unit; i < len; ++i) ref[at + i] = ref[at + i - unit];
        }
        if (rnd(0, 2) == 0)  // N runs of one to five
            for (int k = rnd(1, 4); k > 0; --k) {
                const int len = rnd(1, 5), at = rnd(0, R - len);
                for (int i = 0; i < len; ++i) ref[at + i] = 4;
            }
        bool ref_has[32] = {false};
        for (uint8_t x : ref) ref_has[x] = true;
        SeedParams p{};
        const int K = rnd(3, 6);
        if (!zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, ref_has, K, &p)) continue;
        p.Dn = rnd(0, 4);
        p.Dm = rnd(0, 4);
        p.tol = rnd(0, 8);
        if (rnd(0, 2) == 0) p.spacer += rnd(0, 6);
        const int min_len = rnd(0, 1) ? 0 : rnd(K, 24);
        std::vector<uint32_t> table((size_t)2 << (2 * K), 0);
        zsw::seed_index_build(p, ref.data(), (uint64_t)R, table.data());
        auto geometry = [&](int L) {
            Geometry g;
            g.C = rnd(5, 32);
            g.n_strips = (L + (rnd(0, 4) ? 0 : rnd(1, 40)) + g.C - 1) / g.C;  // a longer lane partner: strips of padding
            g.wu = p.Dn + rnd(0, 24);
            g.wd = p.Dm + rnd(0, 16);
            g.dtmin = -(rnd(0, 3) ? 0 : rnd(0, 32));  // a lane partner's anchor widens the band on one side
            g.dtmax = rnd(0, 3) ? 0 : rnd(0, 32);
            g.R = R;
            return g;
        };
        // the overflow threshold of the call's last tier: a width's own, or anything an unsigned type's bias leaves of it
        // (0: the read's own score + delta, resolved in check_read)
        auto threshold = [&]() { return (long long)(rnd(0, 2) == 0 ? 0 : rnd(0, 1) ? 255 : 65535); };
        for (int k = 0; k < 60 && all_ok; ++k) {
            const int kind = rnd(0, 11);
            std::vector<uint8_t> q = strand_model::gen_read(rnd, ref, K, kind, rnd(K, std::min(R, 90)));
            if (kind == 3) {  // an exact copy: the bounds are reached
                q.clear();
                strand_model::copy_with_errors(rnd, ref, &q, rnd(0, std::max(0, R - 90)), rnd(K, std::min(R, 90)), 0, 0);
            }
            all_ok = check_read(s, p, table, ref, q, min_len, si < 11, geometry((int)q.size()), threshold(), rnd(-3, 3), &cnt);
        }
        for (int k = 0; k < 12 && all_ok; ++k) {  // the structured cases of strand_bound.cpp, each with its own reference
            std::vector<uint8_t> aref, aq;
            SeedParams pa{};
            bool has[32] = {false};
            has[0] = has[1] = has[2] = has[3] = true;
            if (!zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, has, K, &pa)) break;
            pa.Dn = p.Dn;
            pa.Dm = p.Dm;
            pa.tol = p.tol;
            if (!strand_model::far_only_case(rnd, pa, rnd(2 * (K + pa.spacer), 96), &aref, &aq)) continue;
            std::vector<uint32_t> atable((size_t)2 << (2 * K), 0);
            zsw::seed_index_build(pa, aref.data(), (uint64_t)aref.size(), atable.data());
            Geometry g = geometry((int)aq.size());
            g.R = (int)aref.size();
            all_ok = check_read(s, pa, atable, aref, aq, 0, si < 11, g, threshold(), rnd(-3, 3), &cnt);
            ++structured;
        }
    }
    printf("reads %ld (whole-read bound reached %ld), anchored %ld, walks %ld (not accepted %ld, band bound reached %ld); structured cases %ld\n", cnt.reads,
           cnt.whole_tight, cnt.anchored, cnt.walks, cnt.unaccepted, cnt.band_tight, structured);
    if (!all_ok) return 1;
    if (iters >= 100 && (cnt.unaccepted * 10 < cnt.walks || cnt.whole_tight == 0 || cnt.band_tight == 0)) {
        printf("the checks are vacuous: hardly a walk is refused, or no bound is ever reached\n");
        return 1;
    }
    printf("min_score OK\n");
    return 0;
}

// the production setting: which route settles the reads below T. Tier 1 = the band diagonal by diagonal (strips of one column, 8 / 6),
// tier 2 = 48-column strips (25 / 12) for the reads the first tier neither accepts nor settles.
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
    p.Dn = 4;
    p.Dm = 4;
    p.tol = 8;
    std::vector<uint32_t> table((size_t)2 << (2 * K), 0);
    zsw::seed_index_build(p, ref.data(), (uint64_t)R, table.data());
    const int rates[] = {0, 10, 30, 50, 80, 120, 200, 1000}, Ts[] = {150, 200, 225, 250};
    printf("150-base reads against a random 2 kb reference, K = %d, lambda = %d; 2/-5, -10/-1; %d reads per row\n", K, p.lambda, n_reads);
    printf("per T: %% of the reads below T | of those, %% settled by the whole-read bound / a band bound / the exact score of an accepted walk / the full pass\n");
    printf("%-22s", "divergence");
    for (int T : Ts) printf(" | T = %-3d  below:  W   B   A   F", T);
    printf("\n");
    for (int rate : rates) {
        long below[4] = {0}, by_w[4] = {0}, by_b[4] = {0}, by_a[4] = {0}, by_f[4] = {0};
        for (int i = 0; i < n_reads; ++i) {
            std::vector<uint8_t> q;
            if (rate == 1000)
                for (int c = 0; c < L; ++c) q.push_back((uint8_t)rnd(0, 3));
            else
                strand_model::copy_with_errors(rnd, ref, &q, rnd(0, R - L), L, rate, rate / 10);
            auto cell = [&](int c) { return zsw::seed_cell(p, (int)q[c]); };
            auto look = [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
                *f1 = table[2 * (size_t)code];
                *l1 = table[2 * (size_t)code + 1];
            };
            const int truth = strand_model::gotoh(s.w.data(), s.S, s.go, s.ge, ref.data(), R, q.data(), L);
            const zsw::SeedRead sr = zsw::seed_read<true>(p, L, cell, look);
            if (truth > sr.u_whole) {
                printf("claim W violated\n");
                return 1;
            }
            int upper[2] = {0, 0};
            bool acc[2] = {false, false};
            if (sr.ok) {
                const Geometry tiers[2] = {{1, L, 8, 6, sr.dt, sr.dt, R}, {48, (L + 47) / 48, 16 + L / 16, 8 + L / 32, sr.dt, sr.dt, R}};
                for (int k = 0; k < 2; ++k) {
                    const band_model::Walk w = band_model::walk_band(s, p, sr, ref, q, tiers[k], -1, false);
                    upper[k] = zsw::seed_band_upper(w.best2, w.oa, w.ob);
                    acc[k] = !(w.best2 & 1u) && std::max(w.oa, w.ob) <= (int)(w.best2 >> 1);
                    if (truth > upper[k]) {
                        printf("band bound violated\n");
                        return 1;
                    }
                }
            }
            for (int k = 0; k < 4; ++k) {
                const int T = Ts[k];
                if (truth >= T) continue;
                ++below[k];
                if (zsw::seed_below_min(sr.u_whole, T)) ++by_w[k];
                else if (!sr.ok) ++by_f[k];
                else if (acc[0]) ++by_a[k];
                else if (zsw::seed_below_min(upper[0], T)) ++by_b[k];
                else if (acc[1]) ++by_a[k];
                else if (zsw::seed_below_min(upper[1], T)) ++by_b[k];
                else ++by_f[k];
            }
        }
        char name[64];
        if (rate == 1000) snprintf(name, sizeof name, "random reads");
        else snprintf(name, sizeof name, "%.1f %% + %.1f %% indels", rate / 10.0, rate / 100.0);
        printf("%-22s", name);
        for (int k = 0; k < 4; ++k) {
            const double b = (double)std::max(1l, below[k]);
            printf(" | %5.1f %%  %5.1f %5.1f %5.1f %5.1f", 100.0 * below[k] / n_reads, 100.0 * by_w[k] / b, 100.0 * by_b[k] / b, 100.0 * by_a[k] / b, 100.0 * by_f[k] / b);
        }
        printf("\n");
    }
    return 0;
}

}  // namespace

#ifdef ZSW_MIN_SCORE_LIB
// The whole-read bound of each of n reads (residue indices q[offsets[i] .. offsets[i + 1])) as seed_kernel<.., true> derives it: the
// potential of its columns for a read shorter than min_len, seed_read<true>'s u_whole otherwise. Returns -1 if the matrix allows no
// index (the seeded pass then does not run). tests/test_gpu_min_score.py
extern "C" int zsw_model_min_whole(const int32_t* w, int S, int go, int ge, const uint8_t* ref, int R, const uint8_t* q, const int64_t* offsets, int n, int K, int tol,
                                   int min_len, int32_t* out) {
    bool ref_has[32] = {false};
    for (int i = 0; i < R; ++i) ref_has[ref[i] & 31] = true;
    SeedParams p{};
    if (!zsw::seed_analyze(S, w, go, ge, ref_has, K, &p)) return -1;
    p.tol = tol;
    std::vector<uint32_t> table((size_t)2 << (2 * K), 0);
    zsw::seed_index_build(p, ref, (uint64_t)R, table.data());
    for (int i = 0; i < n; ++i) {
        const uint8_t* r = q + offsets[i];
        const int L = (int)(offsets[i + 1] - offsets[i]);
        const zsw::SeedRead sr = zsw::seed_read<true>(
            p, L, [&](int c) { return zsw::seed_cell(p, (int)r[c]); },
            [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
                *f1 = table[2 * (size_t)code];
                *l1 = table[2 * (size_t)code + 1];
            });
        out[i] = L < min_len ? sr.t_all : sr.u_whole;
    }
    return 0;
}
extern "C" int zsw_model_band_upper(uint32_t b2, int oa, int ob) { return zsw::seed_band_upper(b2, oa, ob); }
extern "C" int zsw_model_below_min(long long bound, long long t) { return zsw::seed_below_min(bound, t) ? 1 : 0; }
#else
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "report")) return report(argc > 2 ? atoi(argv[2]) : 1000, argc > 3 ? strtoull(argv[3], nullptr, 10) : 1);
    return run_checks(argc > 1 ? atoi(argv[1]) : 50, argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
}
#endif
