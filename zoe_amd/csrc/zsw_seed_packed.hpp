// zsw_seed_packed.hpp — seed_read (zsw_seed.hpp, the specification) for a block of contiguous reads of one length, in two phases
// (zsw_score_seed.hip: seed_packed_kernel; host model: tests/models/seed_packed.cpp, every field against seed_read).
//
// Phase A converts the block's reads once, eight columns per work item (seed_pack_window, seed_pack8), into rows of 4-bit residue
// codes (15 = padding): the rows the banded pass reads from global memory, and the same rows in LDS for phase B.
// Phase B is one thread per read: seed_read's sweep, column by column, over the read's row — one dword per eight columns, one
// look-up per column in a table of sixteen cells — and behind the sweep the same computation as seed_read with less live state:
// pot_lo | pot_hi << 16 in one word (potentials of at most 65,535: 255 * SEED_PACKED_MAX_LEN), flags as bit masks, `last`
// derived from dhi.
//
// Tried and dropped: a second row of 2-bit k-mer codes and a flag per read, so that a read of good residues only takes its k-mers
// as 2 K bits of that row and its potentials from the layout (47 VGPRs, a tenth of the sweep's instructions). The headline's reads
// carry an N in every second read, so every wavefront ran both forms; and where the two forms met in front of the look-ups the
// compiler kept every array twice (211 VGPRs).
#pragma once
#include "zsw_seed.hpp"

namespace zsw {

constexpr int SEED_PACKED_MAX_LEN = 160;
// LDS row of a read of `len` bases, in dwords from one read's row to the next: a dword per eight columns, odd, so that a
// wavefront's rows fall on distinct banks
ZSW_SEED_HD int seed_packed_res_words(int len) { return ((len + 7) / 8) | 1; }
constexpr int SEED_PACKED_RES_WORDS_MAX = 21;  // seed_packed_res_words(SEED_PACKED_MAX_LEN)

// Eight columns of a read: byte k of w is the read byte of the k-th of them, of which the first ncols (1 .. 8) exist (the other
// bytes may hold anything). entry(byte) = the residue index of the byte (S <= 7 here). Returns the residue codes, 15 for the
// columns that do not exist.
template <class Entry>
ZSW_SEED_HD uint32_t seed_pack8(uint64_t w, int ncols, Entry entry) {
    const uint32_t w0 = (uint32_t)w, w1 = (uint32_t)(w >> 32);
    uint32_t h0 = 0, h1 = 0;  // columns 0-3 / 4-7
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h0 |= (entry((w0 >> (8 * k)) & 0xffu) & 15u) << (4 * k);
        h1 |= (entry((w1 >> (8 * k)) & 0xffu) & 15u) << (4 * k);
    }
    const uint32_t live = ncols < 8 ? (1u << (4 * ncols)) - 1u : 0xffffffffu;  // the columns that exist
    return ((h0 | (h1 << 16)) & live) | ~live;
}

// The eight read bytes of work item (read r, dword d) of a block: src / cnt = the block's bytes (its reads one behind the other,
// len bases each). Column 8 d + k of read r is byte k of the result. Reversed reads (column c = base len - 1 - c) take the eight
// bytes that end at the column's base and swap them. Where the eight would leave the block — the columns that do not exist of its
// first read, reversed, or of its last read — the bytes are fetched one by one and the missing ones are 0.
ZSW_SEED_HD uint64_t seed_pack_window(const uint8_t* src, int cnt, int len, int r, int d, bool rev) {
    const int lo = r * len + (rev ? len - 8 - 8 * d : 8 * d);
    uint64_t w = 0;
    if (lo >= 0 && lo + 8 <= cnt) {
        __builtin_memcpy(&w, src + lo, 8);
    } else {
        for (int b = 0; b < 8; ++b)
            if (lo + b >= 0 && lo + b < cnt) w |= (uint64_t)src[lo + b] << (8 * b);
    }
    return rev ? __builtin_bswap64(w) : w;
}

// seed_span_bound over the packed potentials: pots[i] = pot_lo[i] | pot_hi[i] << 16, bit i of `set` = set[i]
ZSW_SEED_HD int seed_span_bound_packed(int m, const uint32_t* pots, int t_all, uint32_t set, int lambda) {
    int best = 0, cnt = 0;
    int low = 0;
#pragma unroll
    for (int b = 0; b <= SEED_MAX_KMERS; ++b) {
        if (b > m) continue;
        if (b > 0) {
            const int la = (int)(pots[b - 1] & 0xffffu) - lambda * cnt;
            low = la < low ? la : low;
        }
        const int hi = b == m ? t_all : (int)(pots[b < SEED_MAX_KMERS ? b : 0] >> 16);
        const int v = hi - lambda * cnt - low;
        best = v > best ? v : best;
        if (b < m && ((set >> b) & 1u)) ++cnt;
    }
    return best;
}

// seed_vote with the k-mers that do not count moved out of reach: dlo[k] = dhi[k] = SEED_VOTE_FAR for every k >= m and every
// k-mer without an occurrence, so that "within tol of the candidate" is false for them without a test of its own (diagonals lie
// within +- 2^25: the reference has fewer than 2^24 rows). |x - d| <= tol as one unsigned comparison; a candidate that seed_vote
// skips is counted all the same and not taken. Returns seed_vote's (support, *dt): the first candidate in i order with strictly
// larger support.
constexpr int SEED_VOTE_FAR = -(1 << 30);
ZSW_SEED_HD int seed_vote_far(int m, uint32_t has, const int* dlo, const int* dhi, int tol, int* dt) {
    int best = 0, bd = 0;
    const int step = m > 8 ? 2 : 1;
    const uint32_t span = 2u * (uint32_t)tol;
#pragma unroll
    for (int i = 0; i < 2 * SEED_MAX_KMERS; ++i) {
        const int j = i >> 1;
        if (j >= m || (j % step) != 0) continue;
        const int d = (i & 1) ? dhi[j] : dlo[j];
        const bool candidate = ((has >> j) & 1u) && !((i & 1) && dhi[j] == dlo[j]);
        const int e = tol - d;
        int sup = 0;
#pragma unroll
        for (int k = 0; k < SEED_MAX_KMERS; ++k) {
            if (k >= m) continue;
            sup += ((uint32_t)(dlo[k] + e) <= span || (uint32_t)(dhi[k] + e) <= span) ? 1 : 0;
        }
        if (candidate && sup > best) {
            best = sup;
            bd = d;
        }
    }
    *dt = bd;
    return best;
}

// seed_read<WHOLE> of one read of the block. res_row: the read's row as phase A left it; cell16(residue code) = seed_cell of that
// residue; look: the index, as in seed_read. len <= SEED_PACKED_MAX_LEN.
template <bool WHOLE = false, class Cell16, class Lookup>
ZSW_SEED_HD SeedRead seed_read_packed(const SeedParams& p, int len, const uint32_t* res_row, Cell16 cell16, Lookup look) {
    SeedRead out;
    out.ok = 0;
    out.dt = 0;
    out.t_all = 0;
    out.d_fa = 0;
    out.d_bl = 0;
    out.bl_mask = 0;
    out.d_fb = 0;
    out.fa_mask = out.fb_mask = 0;
    int m, stride, c0;
    seed_layout(len, p.K, p.spacer, &m, &stride, &c0);
    const int lam = seed_lambda(p, stride);
    uint32_t pots[SEED_MAX_KMERS], codes[SEED_MAX_KMERS];
    uint32_t usable = 0;
    int pot = 0;
    // seed_read's sweep; the columns come in order, so a row's dword is fetched once per eight of them
    uint32_t word = 0;
    auto cell = [&](int c) {
        if ((c & 7) == 0) word = res_row[c >> 3];
        return cell16((word >> (4 * (c & 7))) & 15u);
    };
    int c = 0;
#pragma unroll
    for (int j = 0; j < SEED_MAX_KMERS; ++j) {
        pots[j] = codes[j] = 0;
        if (j >= m) continue;
        const int cj = c0 + j * stride;
        int run = p.ins_col;
        for (; c < cj; ++c) {
            const int wpc = (int)(cell(c) & 0xffu);
            pot += wpc;
            run += wpc + p.ge;
        }
        uint32_t code = 0, lo = 0, hi = 0;
        bool ok = j == 0 || run >= lam;
        for (int k = 0; k < p.K; ++k, ++c) {
            const uint32_t x = cell(c);
            pot += (int)(x & 0xffu);
            ok = ok && (x >> 8) != 0xffu;
            code |= ((x >> 8) & 3u) << (2 * k);
            if (k == 0) lo = (uint32_t)pot;
            if (k == p.K - 2) hi = (uint32_t)pot;
        }
        pots[j] = lo | (hi << 16);
        if (ok) {
            usable |= 1u << j;
            codes[j] = code;
        }
    }
    for (; c < len; ++c) pot += (int)(cell(c) & 0xffu);
    // the index entries, sixteen loads in flight; a k-mer's diagonals take the place of its entry
    uint32_t f1s[SEED_MAX_KMERS], l1s[SEED_MAX_KMERS];
#pragma unroll
    for (int j = 0; j < SEED_MAX_KMERS; ++j) {
        f1s[j] = l1s[j] = 0;
        look(codes[j], &f1s[j], &l1s[j]);
    }
    int dlo[SEED_MAX_KMERS], dhi[SEED_MAX_KMERS];
    bool hasb[SEED_MAX_KMERS];
    uint32_t has = 0;
#pragma unroll
    for (int j = 0; j < SEED_MAX_KMERS; ++j) {
        const int cj = c0 + j * stride;
        hasb[j] = ((usable >> j) & 1u) && f1s[j] != 0;  // (usable holds bits below m only)
        has |= hasb[j] ? 1u << j : 0u;
        dlo[j] = hasb[j] ? (int)(f1s[j] - 1) - cj : SEED_VOTE_FAR;
        dhi[j] = hasb[j] ? (int)(l1s[j] - 1) - cj : SEED_VOTE_FAR;
    }
    out.t_all = pot;
    out.u_whole = pot;
    if (m == 0) return out;
    if (WHOLE) out.u_whole = seed_span_bound_packed(m, pots, pot, usable & ~has, lam);
    int dt = 0;
    const int support = seed_vote_far(m, has, dlo, dhi, p.tol, &dt);
    if (support < (m >= 3 ? 2 : 1)) return out;
#pragma unroll
    for (int i = 0; i < SEED_MAX_KMERS; ++i) {
        const int ci = c0 + i * stride;
        const bool u = (usable >> i) & 1u;
        out.fa_mask |= (u && (!hasb[i] || dlo[i] >= dt - p.Dn)) ? 1u << i : 0u;
        out.bl_mask |= (u && (!hasb[i] || dhi[i] + ci < dt + len + p.M2)) ? 1u << i : 0u;  // (last occurrence = dhi + the k-mer's column)
        out.fb_mask |= (u && (!hasb[i] || dhi[i] <= dt + p.Dm)) ? 1u << i : 0u;
    }
    const int u_fa = seed_span_bound_packed(m, pots, pot, out.fa_mask, lam);
    const int u_bl = seed_span_bound_packed(m, pots, pot, out.bl_mask, lam);
    const int u_fb = seed_span_bound_packed(m, pots, pot, out.fb_mask, lam);
    out.ok = 1;
    out.dt = dt;
    out.d_fa = pot - u_fa > 255 ? 255 : pot - u_fa;
    out.d_bl = pot - u_bl > 255 ? 255 : pot - u_bl;
    out.d_fb = pot - u_fb > 255 ? 255 : pot - u_fb;
    return out;
}

}  // namespace zsw
