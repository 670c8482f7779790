// seed_diag.cpp — host model of the diagonal first tier (seed_diag_kernel, zoe_amd/csrc/zsw_score_band.hip): the banded pass of
// seed_band.cpp with strips of ONE column, where the band is exactly wu + wd + 1 (+ the distance of the lane partners' anchors)
// diagonals and nothing else. Three parts:
//   1. the cell-by-cell checks of seed_band.cpp (I1, O1-O3, the per-class checks, A) at C = 1 — that model's own generator draws
//      strips of 5-64 columns only;
//   2. a twin of the kernel's walk in plain integers — a register per DIAGONAL, one column per step, E running down the column,
//      the neutral table entry outside the reference, the column masks of a 16-column group, the spare diagonal below the band of a
//      pair with one anchor — whose (maximum, oa, ob) must EQUAL the strip walk's at C = 1 on every read;
//   3. zsw_seed_diag.hpp: seed_free_bits against seed_exit_is_free column by column.
// usage: seed_diag <iterations> <seed>
#define ZSW_MODEL_LIB
#include "seed_band.cpp"

#include "../../zoe_amd/csrc/zsw_seed_diag.hpp"

namespace {

constexpr int GROUP = 16;  // the kernel's unrolled columns: one set of column masks per group

struct DiagWalk {
    uint32_t best2 = 0;
    int oa = 0, ob = 0;
};

// The kernel's walk over one read. spare: the window has one diagonal more than the band (a pair whose anchors coincide): it
// stands for the cells below the band.
DiagWalk walk_diag(const Scheme& s, const SeedParams& p, const zsw::SeedRead& sr, const std::vector<uint8_t>& ref, const std::vector<uint8_t>& q, const Geometry& g,
                   int tag, bool spare) {
    const int R = g.R, L = (int)q.size(), n_cols = g.n_strips;
    const int D = g.wu + g.wd + 1 + (g.dtmax - g.dtmin) + (spare ? 1 : 0), last = spare ? D - 2 : D - 1;
    const Layout y = layout_of(p, L);
    const int base = g.dtmin - g.wu, go2 = 2 * s.go, ge2 = 2 * s.ge;
    zsw::SeedColDP up, lo;
    zsw::seed_col_init(&up);
    zsw::seed_col_init(&lo);
    std::vector<int64_t> H(D, 0), F(D, 0);
    int64_t Fbelow = 0;
    DiagWalk out;
    for (int k0 = 0; k0 < n_cols; k0 += GROUP) {
        const zsw::SeedStripEvents ea = zsw::seed_strip_events(k0, GROUP, y.m, y.c0, y.stride, p.K, y.magic, sr.fa_mask);
        const zsw::SeedStripEvents eb = zsw::seed_strip_events(k0, GROUP, y.m, y.c0, y.stride, p.K, y.magic, sr.fb_mask);
        const uint32_t freeb = zsw::seed_free_bits(k0, GROUP, y.m, y.c0, y.stride, p.K, p.spacer, y.magic, sr.fa_mask);
        const int t0 = base + k0, t1 = g.dtmax + k0 + 1 + g.wd;
        const uint32_t above = zsw::seed_bits_from(1 - t0), below = zsw::seed_bits_below(R - t1);
        const uint32_t topin = zsw::seed_bits_from(-t0) & zsw::seed_bits_below(R - t0);
        const uint32_t exits = below & zsw::seed_bits_from(1 - t1), yfok = below & zsw::seed_bits_from(-t1);
        const uint32_t real = zsw::seed_bits_below(L - k0);
        const uint32_t inj = real & above, join = zsw::seed_bits_below(L - k0 - 1) & topin, ex = real & exits, bel = real & below, nm = real & yfok;
        for (int u = 0; u < GROUP && k0 + u < n_cols; ++u) {
            const int k = k0 + u;
            auto bit = [&](uint32_t x) { return ((x >> u) & 1u) != 0; };
            int a = 0;
            if (k < L) a = zsw::seed_col_step(&up, p.maxw, y.lam, bit(ea.start), bit(ea.end));
            const int v = bit(inj) ? std::max(a, 0) : 0;
            out.oa = std::max(out.oa, v);
            int64_t E = bit(topin) ? zsw::seed_tag(std::max(0, v - s.go), tag) : 0;
            int64_t rmax = 0;
            for (int j = 0; j < D; ++j) {
                const int r = base + k + j;
                const int wgt = (r >= 0 && r < R && k < L) ? 2 * s.w[ref[r] * s.S + q[k]] : 0;  // the neutral entry, padding columns
                const int64_t hd = H[j] + wgt, Fin = j + 1 < D ? F[j + 1] : Fbelow;
                const int64_t h = std::max(std::max(hd, E), Fin);
                H[j] = h;
                F[j] = std::max<int64_t>(std::max(Fin - ge2, h - go2), 0);
                E = std::max<int64_t>(std::max(E - ge2, h - go2), 0);
                if (j <= last) rmax = std::max(rmax, h);
            }
            out.best2 = (uint32_t)std::max<int64_t>(out.best2, rmax);
            if (bit(join)) zsw::seed_col_join(&up, zsw::seed_untag((uint32_t)H[0], tag), bit(freeb));
            int b = 0;
            if (k < L) b = zsw::seed_col_step(&lo, p.maxw, y.lam, bit(eb.start), bit(eb.end));
            if (bit(ex)) {
                const int he = zsw::seed_untag((uint32_t)H[last], tag);
                zsw::seed_col_join(&lo, he, bit(eb.inside));
                b = std::max(b, he);
            }
            b = std::max(b, 0);
            if (bit(bel)) out.ob = std::max(out.ob, b);
            Fbelow = zsw::seed_tag(bit(nm) ? std::max(0, b + std::max(0, y.lam - p.maxw) - s.go) : 0, tag);
            if (spare) F[D - 1] = Fbelow;
        }
    }
    return out;
}

bool check_twin(const Scheme& s, const SeedParams& p, const std::vector<uint32_t>& table, const std::vector<uint8_t>& ref, const std::vector<uint8_t>& q, int wu, int wd,
                int slo, int shi, int extra, long* compared) {
    const int L = (int)q.size();
    auto cell = [&](int c) { return zsw::seed_cell(p, (int)q[c]); };
    auto look = [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
        *f1 = table[2 * (size_t)code];
        *l1 = table[2 * (size_t)code + 1];
    };
    const zsw::SeedRead sr = zsw::seed_read(p, L, cell, look);
    if (!sr.ok) return true;
    const Geometry g{1, L + extra, wu, wd, sr.dt - slo, sr.dt + shi, (int)ref.size()};
    for (int tag = -1; tag <= 1; tag += 2)
        for (int spare = 0; spare < 2; ++spare) {
            const Walk w = walk_band(s, p, sr, ref, q, g, tag, false);
            const DiagWalk d = walk_diag(s, p, sr, ref, q, g, tag, spare != 0);
            ++*compared;
            if (d.best2 != w.best2 || d.oa != std::max(w.oa, 0) || d.ob != std::max(w.ob, 0)) {
                printf("twin: (maximum2, oa, ob) diagonal walk (%u, %d, %d), strip walk at C = 1 (%u, %d, %d); tag %d spare %d dt %d wu %d wd %d dtmin %d dtmax %d cols %d R %d L %d\n",
                       d.best2, d.oa, d.ob, w.best2, std::max(w.oa, 0), std::max(w.ob, 0), tag, spare, sr.dt, wu, wd, g.dtmin, g.dtmax, g.n_strips, g.R, L);
                return false;
            }
        }
    return true;
}

bool check_free_bits(std::mt19937_64& rng) {
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int it = 0; it < 400; ++it) {
        const int K = rnd(3, 12), spacer = rnd(2, 9), L = rnd(K, 300), n = rnd(1, 32);
        int m, stride, c0;
        zsw::seed_layout(L, K, spacer, &m, &stride, &c0);
        const uint32_t magic = zsw::seed_div_magic(stride), mask = (uint32_t)rng() & 0xffffu;
        for (int k0 = 0; k0 < L + 40; k0 += rnd(1, n)) {
            const uint32_t bits = zsw::seed_free_bits(k0, n, m, c0, stride, K, spacer, magic, mask);
            for (int i = 0; i < 32; ++i) {
                const bool want = i < n && zsw::seed_exit_is_free(k0 + i, m, c0, stride, K, spacer, magic, mask);
                if ((((bits >> i) & 1u) != 0) != want) {
                    printf("seed_free_bits(k0 %d, n %d) bit %d is %d, seed_exit_is_free says %d (L %d K %d spacer %d mask %x)\n", k0, n, i, (int)((bits >> i) & 1u), (int)want, L, K,
                           spacer, mask);
                    return false;
                }
            }
        }
    }
    for (int t = -40; t <= 40; ++t)
        for (int i = 0; i < 32; ++i)
            if ((((zsw::seed_bits_from(t) >> i) & 1u) != 0) != (i >= t) || (((zsw::seed_bits_below(t) >> i) & 1u) != 0) != (i < t)) {
                printf("seed_bits_from / seed_bits_below (%d) bit %d\n", t, i);
                return false;
            }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 50;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    if (!check_free_bits(rng)) return 1;
    const Scheme schemes[] = {dna(2, -5, 0, 10, 1), dna(1, -1, 0, 2, 1), dna(3, -2, 0, 5, 0), dna(1, -3, 0, 5, 2), dna(5, -4, 0, 8, 0),
                              dna(2, -5, -1, 10, 1), dna(4, -6, 1, 12, 2), dna(2, -2, 0, 3, 3), dna(2, -10, 0, 10, 1), dna(2, -5, 0, 5, 1),
                              dna(3, -9, 0, 6, 1)};
    constexpr int SLACK = 1;  // SEED_DIAG_SLACK: lane partners up to the slack apart, and one beyond it
    Counters cnt;
    long structured = 0, twins = 0;
    bool all_ok = true;
    for (int it = 0; it < iters && all_ok; ++it) {
        const Scheme& s = schemes[it % (sizeof(schemes) / sizeof(schemes[0]))];
        const int R = rnd(60, 420);
        std::vector<uint8_t> ref(R);
        for (auto& x : ref) x = (uint8_t)rnd(0, 3);
        if (rnd(0, 2) == 0 && R > 120) {
            const int len = rnd(20, 50), from = rnd(0, R - len), to = rnd(0, R - len);
            for (int i = 0; i < len; ++i) ref[to + i] = ref[from + i];
        }
        if (rnd(0, 3) == 0 && R > 100) {
            const int unit = rnd(1, 6), len = rnd(20, 60), at = rnd(0, R - len);
            for (int i = unit; i < len; ++i) ref[at + i] = ref[at + i - unit];
        }
        if (rnd(0, 3) == 0)
            for (int k = rnd(1, 6); k > 0; --k) ref[rnd(0, R - 1)] = 4;
        bool ref_has[32] = {false};
        for (uint8_t x : ref) ref_has[x] = true;
        SeedParams p;
        const int K = rnd(3, 6);
        if (!zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, ref_has, K, &p)) continue;
        p.M1 = p.M1_per8 = p.M2 = p.Wd = p.Wd_per16 = 0;
        p.Dn = rnd(0, 4);
        p.Dm = rnd(0, 4);
        p.tol = rnd(0, 5);
        if (rnd(0, 2) == 0) p.spacer += rnd(0, 6);
        std::vector<uint32_t> table((size_t)2 << (2 * K), 0);
        zsw::seed_index_build(p, ref.data(), (uint64_t)R, table.data());
        auto geometry = [&](int* wu, int* wd, int* slo, int* shi, int* extra) {
            *wu = p.Dn + (rnd(0, 2) ? rnd(0, 6) : rnd(0, 24));  // (the kernel: 8 and 6)
            *wd = p.Dm + (rnd(0, 2) ? rnd(0, 4) : rnd(0, 16));
            *slo = rnd(0, 2) ? 0 : rnd(0, SLACK + 1);
            *shi = rnd(0, 2) ? 0 : rnd(0, SLACK + 1);
            *extra = rnd(0, 3) ? 0 : rnd(1, 40);  // a longer lane partner: columns of padding
        };
        for (int k = 0; k < 60 && all_ok; ++k) {
            const int kind = rnd(0, 12);
            const int L = rnd(K, std::min(R, 90));
            std::vector<uint8_t> q;
            auto copy_with_errors = [&](int start, int len, int sub_pm, int indel_pm) {  // per mille
                int i = start;
                while ((int)q.size() < len) {
                    uint8_t b = (i >= 0 && i < R) ? ref[i] : (uint8_t)rnd(0, 3);
                    const int e = rnd(0, 999);
                    if (e < sub_pm) b = (uint8_t)((b + rnd(1, 3)) & 3);
                    else if (e < sub_pm + indel_pm / 2) { ++i; continue; }
                    else if (e < sub_pm + indel_pm) { q.push_back((uint8_t)rnd(0, 3)); continue; }
                    q.push_back(b);
                    ++i;
                }
                q.resize(len);
            };
            int div_class = -1;
            if (kind <= 3) copy_with_errors(rnd(0, std::max(0, R - L)), L, rnd(0, 30), rnd(0, 10));
            else if (kind == 4 || kind == 11 || kind == 12) {
                static const int rate[4] = {30, 50, 80, 120};
                div_class = rnd(0, 3);
                copy_with_errors(rnd(0, std::max(0, R - L)), L, rate[div_class], rate[div_class] / 10);
            } else if (kind == 5) copy_with_errors(rnd(0, std::max(0, R - L)), L, rnd(50, 200), rnd(10, 50));
            else if (kind == 6) {  // a chimera
                const int l1 = rnd(K, std::max(K, L - 1));
                copy_with_errors(rnd(0, std::max(0, R - l1)), l1, 10, 0);
                copy_with_errors(rnd(0, std::max(0, R - L)), L, 10, 0);
            } else if (kind == 7 || kind == 9) copy_with_errors(rnd(0, 1) ? -rnd(1, L / 2 + 1) : R - rnd(1, L / 2 + 1) - L / 2, L, 10, 0);  // over either end of the reference
            else if (kind == 8) {  // a long deletion / insertion
                const int l1 = L / 2, st = rnd(0, std::max(0, R - L - 30));
                copy_with_errors(st, l1, 0, 0);
                if (rnd(0, 1)) {
                    int i = st + l1 + rnd(3, 28);
                    while ((int)q.size() < L) q.push_back(i < R ? ref[i++] : (uint8_t)rnd(0, 3));
                } else {
                    for (int x = rnd(3, 20); x > 0 && (int)q.size() < L; --x) q.push_back((uint8_t)rnd(0, 3));
                    int i = st + l1;
                    while ((int)q.size() < L) q.push_back(i < R ? ref[i++] : (uint8_t)rnd(0, 3));
                }
            } else copy_with_errors(rnd(0, std::max(0, R - L)), L, 0, 0);  // an exact copy: every detour out of the band and back is open
            if (rnd(0, 4) == 0)
                for (int x = rnd(1, 3); x > 0; --x) q[rnd(0, L - 1)] = 4;
            int wu, wd, slo, shi, extra;
            geometry(&wu, &wd, &slo, &shi, &extra);
            all_ok = check_read(s, p, table, ref, q, kind <= 3, div_class, 1, wu, wd, slo, shi, extra, &cnt) && check_twin(s, p, table, ref, q, wu, wd, slo, shi, extra, &twins);
        }
        for (int k = 0; k < 12 && all_ok; ++k) {  // structured cases (adversarial_reads.hpp), each with its own reference
            std::vector<uint8_t> aref, aq;
            SeedParams pa;
            bool has[32] = {false};
            has[0] = has[1] = has[2] = has[3] = true;
            if (!zsw::seed_analyze(s.S, s.w.data(), s.go, s.ge, has, K, &pa)) break;
            pa.M1 = pa.M1_per8 = pa.M2 = pa.Wd = pa.Wd_per16 = 0;
            pa.Dn = p.Dn;
            pa.Dm = p.Dm;
            pa.tol = p.tol;
            if (!adversarial::spacer_case(rng, pa, rnd(2 * (K + pa.spacer), 96), &aref, &aq)) continue;
            std::vector<uint32_t> atable((size_t)2 << (2 * K), 0);
            zsw::seed_index_build(pa, aref.data(), (uint64_t)aref.size(), atable.data());
            Counters unused;
            int wu, wd, slo, shi, extra;
            geometry(&wu, &wd, &slo, &shi, &extra);
            all_ok = check_read(s, pa, atable, aref, aq, false, -1, 1, wu, wd, slo, shi, extra, &unused) && check_twin(s, pa, atable, aref, aq, wu, wd, slo, shi, extra, &twins);
            ++structured;
        }
    }
    printf("reads %ld, anchored %ld, accepted (score) %ld, accepted (ends) %ld; plain reads %ld, of which accepted %ld; structured cases %ld; twin walks compared %ld\n", cnt.reads,
           cnt.anchored, cnt.pass_score, cnt.pass_ends, cnt.plain, cnt.plain_pass, structured, twins);
    printf("diverged reads accepted (3 / 5 / 8 / 12 %% substitutions): %ld/%ld %ld/%ld %ld/%ld %ld/%ld\n", cnt.div_pass[0], cnt.div_reads[0], cnt.div_pass[1],
           cnt.div_reads[1], cnt.div_pass[2], cnt.div_reads[2], cnt.div_pass[3], cnt.div_reads[3]);
    if (!all_ok) return 1;
    if (cnt.plain > 200 && cnt.plain_pass * 5 < cnt.plain) {
        printf("the checks are vacuous: fewer than a fifth of the plain reads are accepted\n");
        return 1;
    }
    if (twins < 100) {
        printf("the checks are vacuous: next to no twin walks\n");
        return 1;
    }
    printf("seed_diag OK\n");
    return 0;
}
