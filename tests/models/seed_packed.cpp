// seed_packed.cpp — host check of the two-phase seed kernel's arithmetic (zoe_amd/csrc/zsw_seed_packed.hpp, what
// seed_packed_kernel runs) against the specification, seed_read (zsw_seed.hpp). Blocks of reads of one length are laid out as the
// kernel sees them — one behind the other, in a buffer of exactly their bytes — and converted work item by work item as in its
// phase A (seed_pack_window, seed_pack8, rows at the kernel's stride); then, read by read:
//   1. the residue-code dwords equal what seed_kernel writes today: base by base, 15 in the columns behind the read, 0xffffffff
//      in the row's last dword;
//   2. seed_read_packed returns every field of seed_read, with and without WHOLE (u_whole) — the vote (seed_vote_far) included.
// Exhaustive over the layouts: every length min_len .. max_len, K = 8 .. 12, spacer 2 .. 4, both orientations, two potential
// tables (N has potential 0 / 1) plus a matrix whose good residues do not all have the potential maxw and whose 2-bit codes are
// not the residue indices; references of 60, 300 and 2,000 bases with a repeat, so that first and last occurrences differ often and
// the vote has ties to break. Reads: pieces of the reference with substitutions; one N, a run of N, bytes outside the alphabet —
// anywhere, and just before, inside and just behind a sampled k-mer; unrelated reads.
// usage: seed_packed <min_len> <max_len> [reads per layout] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zoe_amd/csrc/zsw_seed_packed.hpp"

namespace {

using zsw::SeedParams;
using zsw::SeedRead;


struct Config {
    SeedParams p;
    uint8_t index_map[256];
    const char* name;
};

Config make_config(int K, int spacer, int variant) {
    Config c;
    memset(&c, 0, sizeof c);
    SeedParams& p = c.p;
    for (int q = 0; q < 32; ++q) {
        p.code[q] = 0xff;
        p.wp[q] = 0;
    }
    p.K = K;
    p.maxw = 2;
    p.lambda = 7;
    p.go = 10;
    p.ge = 1;
    p.ins_col = p.maxw + p.ge;
    p.spacer = spacer;
    p.M1 = 24;
    p.M1_per8 = 1;
    p.M2 = 16;
    p.Dn = 4;
    p.Dm = 4;
    p.Wd = 9;
    p.Wd_per16 = 1;
    p.tol = 8;
    for (int q = 0; q < 4; ++q) {
        p.code[q] = (uint8_t)q;
        p.wp[q] = 2;
    }
    c.name = "N has potential 0";
    if (variant == 1) {
        p.wp[4] = 1;
        c.name = "N has potential 1";
    }
    if (variant == 2) {  // codes that are not the indices, a good residue below maxw, a catch-all with a potential
        const uint8_t perm[4] = {2, 0, 3, 1};
        for (int q = 0; q < 4; ++q) p.code[q] = perm[q];
        p.wp[2] = 1;
        p.wp[4] = 1;
        p.wp[5] = 2;
        c.name = "permuted codes";
    }
    for (int b = 0; b < 256; ++b) c.index_map[b] = 5;
    c.index_map['A'] = 0;
    c.index_map['C'] = 1;
    c.index_map['G'] = 2;
    c.index_map['T'] = 3;
    c.index_map['N'] = 4;
    return c;
}

struct Rng {
    std::mt19937_64 g;
    int below(int n) { return (int)(g() % (uint64_t)n); }
};

const uint8_t ACGT[4] = {'A', 'C', 'G', 'T'};

bool same(const SeedRead& a, const SeedRead& b, bool whole) {
    return a.ok == b.ok && a.dt == b.dt && a.t_all == b.t_all && a.d_fa == b.d_fa && a.d_bl == b.d_bl && a.bl_mask == b.bl_mask && a.d_fb == b.d_fb &&
           a.fa_mask == b.fa_mask && a.fb_mask == b.fb_mask && (!whole || a.u_whole == b.u_whole) && (whole || a.u_whole == a.t_all);
}

void show(const char* who, const SeedRead& r) {
    printf("  %s: ok %d dt %d t_all %d d_fa %d d_bl %d d_fb %d bl %04x fa %04x fb %04x u_whole %d\n", who, r.ok, r.dt, r.t_all, r.d_fa, r.d_bl, r.d_fb, r.bl_mask, r.fa_mask,
           r.fb_mask, r.u_whole);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        printf("usage: seed_packed <min_len> <max_len> [reads per layout] [seed]\n");
        return 2;
    }
    const int min_len = atoi(argv[1]), max_len = atoi(argv[2]);
    const int per = argc > 3 ? atoi(argv[3]) : 24;
    Rng rng{std::mt19937_64(argc > 4 ? strtoull(argv[4], nullptr, 10) : 1)};
    if (min_len < 1 || max_len > zsw::SEED_PACKED_MAX_LEN || min_len > max_len || per < 1) return 2;
    const int ref_lens[3] = {60, 300, 2000};
    long long n_reads = 0, n_plain = 0, n_anchored = 0, n_split = 0;
    for (int K = 8; K <= 12; ++K) {
        std::vector<uint32_t> table((size_t)2 << (2 * K));
        for (int variant = 0; variant < 3; ++variant) {
            for (int ri = 0; ri < 3; ++ri) {
                // the reference: random, with a repeat (first != last occurrence) and a few N
                const int R = ref_lens[ri];
                std::vector<uint8_t> ref(R);
                for (int i = 0; i < R; ++i) ref[i] = ACGT[rng.below(4)];
                for (int i = 0; i < R / 4; ++i) ref[R / 2 + i] = ref[i];
                for (int i = 0; i < R / 100; ++i) ref[rng.below(R)] = 'N';
                Config cfg = make_config(K, 2, variant);
                std::vector<uint8_t> ref_idx(R);
                for (int i = 0; i < R; ++i) ref_idx[i] = cfg.index_map[ref[i]];
                std::fill(table.begin(), table.end(), 0u);
                zsw::seed_index_build(cfg.p, ref_idx.data(), (uint64_t)R, table.data());
                auto look = [&](uint32_t code, uint32_t* f1, uint32_t* l1) {
                    *f1 = table[2 * (size_t)code];
                    *l1 = table[2 * (size_t)code + 1];
                };
                for (int spacer = 2; spacer <= 4; ++spacer) {
                    cfg.p.spacer = spacer;
                    const SeedParams& p = cfg.p;
                    // the lengths are shared out over the references: every length meets every K, spacer, variant and orientation
                    for (int L = min_len + ri; L <= max_len; L += 3) {
                        int m, stride, c0;
                        zsw::seed_layout(L, K, spacer, &m, &stride, &c0);
                        const int nr = per;
                        std::vector<uint8_t> block((size_t)nr * L);  // exactly the block's bytes: a byte fetched outside is an error
                        for (int rev = 0; rev < 2; ++rev) {
                            for (int r = 0; r < nr; ++r) {
                                uint8_t* q = block.data() + (size_t)r * L;
                                const int kind = r % 8;
                                if (kind == 7) {
                                    for (int i = 0; i < L; ++i) q[i] = ACGT[rng.below(4)];
                                } else {  // a piece of the reference (wrapped around a short one), 0 .. 5 % substituted
                                    const int at = rng.below(R);
                                    for (int i = 0; i < L; ++i) q[rev ? L - 1 - i : i] = ref[(at + i) % R];
                                    const int pc = rng.below(6);
                                    for (int i = 0; i < L; ++i)
                                        if (rng.below(100) < pc) q[i] = ACGT[rng.below(4)];
                                }
                                // column c of the read is byte (rev ? L - 1 - c : c)
                                auto put = [&](int c, uint8_t b) {
                                    if (c >= 0 && c < L) q[rev ? L - 1 - c : c] = b;
                                };
                                const int j = m ? rng.below(m) : 0, cj = c0 + j * stride;
                                const uint8_t odd = (r & 8) ? (uint8_t)(rng.below(2) ? 'X' : 0xff) : (uint8_t)'N';
                                if (kind == 1) put(rng.below(L), odd);
                                if (kind == 2) {
                                    const int at = rng.below(L), run = 1 + rng.below(20);
                                    for (int i = 0; i < run; ++i) put(at + i, odd);
                                }
                                if (kind == 3) put(cj - 1, odd);
                                if (kind == 4) put(cj + rng.below(K), odd);
                                if (kind == 5) put(cj + K, odd);
                                if (kind == 6) {
                                    put(cj + K - 1, odd);
                                    put(rng.below(L), 'N');
                                }
                            }
                            // phase A, item by item, with the kernel's strides and the banded pass's row stride cs
                            const int cs = (L + 7) / 8 + 1, rw = (L + 7) / 8;
                            const int res_words = zsw::seed_packed_res_words(L);
                            if (res_words < rw || !(res_words & 1) || res_words > zsw::SEED_PACKED_RES_WORDS_MAX) {
                                printf("L %d: a row stride of %d does not hold the row\n", L, res_words);
                                return 1;
                            }
                            std::vector<uint32_t> res_rows((size_t)nr * res_words, 0xdeadbeefu), codes_out((size_t)nr * cs, 0u);
                            const uint32_t magic = zsw::seed_div_magic(cs);
                            for (int i = 0; i < nr * cs; ++i) {
                                const int r = zsw::seed_div(i, magic), d = i - r * cs;
                                if (r != i / cs) {
                                    printf("seed_div(%d, %d) = %d\n", i, cs, r);
                                    return 1;
                                }
                                uint32_t res = 0xffffffffu;
                                if (d < rw) {
                                    const int ncols = L - 8 * d < 8 ? L - 8 * d : 8;
                                    const uint64_t w = zsw::seed_pack_window(block.data(), nr * L, L, r, d, rev != 0);
                                    res = zsw::seed_pack8(w, ncols, [&](uint32_t b) { return (uint32_t)cfg.index_map[b]; });
                                    res_rows[(size_t)r * res_words + d] = res;
                                }
                                codes_out[i] = res;
                            }
                            for (int r = 0; r < nr; ++r) {
                                const uint8_t* q = block.data() + (size_t)r * L;
                                auto residue = [&](int c) { return (int)cfg.index_map[q[rev ? L - 1 - c : c]]; };
                                // 1. the residue codes, as seed_kernel packs them
                                bool any = false;
                                for (int c = 0; c < 8 * cs; ++c) {
                                    const uint32_t got = (codes_out[(size_t)r * cs + (c >> 3)] >> (4 * (c & 7))) & 15u;
                                    const uint32_t want = c < L ? (uint32_t)(residue(c) & 15) : 15u;
                                    if (got != want) {
                                        printf("L %d K %d rev %d read %d column %d: residue code %u, want %u\n", L, K, rev, r, c, got, want);
                                        return 1;
                                    }
                                    if (c < L && !(p.code[residue(c)] != 0xff && p.wp[residue(c)] == p.maxw)) any = true;
                                }
                                // 2. every field
                                auto cell = [&](int c) { return zsw::seed_cell(p, residue(c)); };
                                auto cell16 = [&](uint32_t res) { return zsw::seed_cell(p, (int)res); };
                                const uint32_t* rr = res_rows.data() + (size_t)r * res_words;
                                const SeedRead want0 = zsw::seed_read<false>(p, L, cell, look), want1 = zsw::seed_read<true>(p, L, cell, look);
                                const SeedRead got0 = zsw::seed_read_packed<false>(p, L, rr, cell16, look), got1 = zsw::seed_read_packed<true>(p, L, rr, cell16, look);
                                if (!same(got0, want0, false) || !same(got1, want1, true)) {
                                    printf("%s, L %d K %d spacer %d rev %d reference %d read %d:\n", cfg.name, L, K, spacer, rev, R, r);
                                    show("seed_read        ", want0);
                                    show("seed_read_packed ", got0);
                                    show("seed_read<W>     ", want1);
                                    show("seed_read_packed<W>", got1);
                                    return 1;
                                }
                                ++n_reads;
                                n_plain += !any;
                                n_anchored += want0.ok;
                                // (how often the vote had a k-mer with two occurrences to weigh)
                                n_split += want0.ok && (want0.fa_mask != want0.fb_mask);
                            }
                        }
                    }
                }
            }
        }
    }
    printf("%lld reads, %lld of good residues only, %lld anchored, %lld with different masks left and right\n", n_reads, n_plain, n_anchored, n_split);
    if (n_plain * 10 < n_reads || (n_reads - n_plain) * 10 < n_reads || n_anchored * 4 < n_reads || n_split == 0) {
        printf("the reads do not exercise both kinds of reads, the anchors and the masks\n");
        return 1;
    }
    printf("seed_packed OK\n");
    return 0;
}
