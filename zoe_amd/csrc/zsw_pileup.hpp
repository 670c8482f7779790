// zsw_pileup.hpp — the rules of zsw_pileup_batch and zsw_consensus_from_counts (include/zoe_sw.h), shared as text by the kernels
// (zsw_pileup.hip) and the host model (tests/models/pileup_walk.cpp): the records of an alignment call reduced to one table over the
// context's sequence — per site, how often each of eight byte classes stood opposite it —, and the plurality base of every site.
//   which read byte meets which site   pairwise_align_with (src/alignment/pairwise.rs:26-65): M = X pair a byte of each sequence,
//                                      D puts `-` and N puts `N` opposite the record's reference, I puts query bytes opposite nothing
//   the bins                           NucleotideCounts (src/composition/by_position/mod.rs), in the order of into_inner()
//   the vote                           NucleotideCounts::plurality_acgtn
//
// A record contributes all of its columns or none: validate() goes over the ciglets alone — the checks of zsw_annotate.hpp's walk
// that do not need a base: record_ok(), no inc of 0, no op outside MIDNSHP=X, no ciglet that leaves either sequence — before count()
// touches a counter. (The merged-inc overflow of the verbose CIGAR is no check here: nothing is merged.)
//
// count() does not add 1 per column. Three of the four things a ciglet can do are range adds — `inc` gaps, `inc` N, and `inc`
// columns that are "covered as expected": the read's byte falls in the bin of the sequence's own byte — and a range add is +1 at its
// first site and -1 one past its last in a difference array of len + 1 entries. Only columns whose bin differs from the sequence's
// are touched one by one: miss[site] += 1, counts[site][bin] += 1. resolve_site(), given the prefix sums of the three difference
// arrays, adds cover - miss into the sequence's own bin, the gaps into bin 5 and the N into bin 4. Every column takes exactly one
// of the two routes, all arithmetic is modulo 2^32, and addition commutes: the table is exact and the same on every run.
//
// Both walks are written as code that every lane of a group of PILEUP_G lanes executes with the same values; what differs per
// lane sits behind the Io object:
//   io.ciglet(k, &inc, &op)       ciglet k of the record
//   io.range(which, site, n)      difference array `which`: +1 at site, -1 at site + n
//   io.columns(site, rd, nv)      sites site + l opposite read bytes rd + l for l < nv <= PILEUP_G: the miss route where the bins differ
//   io.insertion(p, n)            ins[p].runs += 1, ins[p].bases += n (if the table was asked for)
// The kernel's Io is a wavefront, the model's Io loops over the lanes.
//
// While the accumulators of a sequence (Diff, 16 bytes per site, plus one byte per site for the sequence's bins) fit
// PILEUP_LDS_SITES_MAX sites, every block keeps its own in LDS and adds them to the global workspace once, at its end. The constant
// comes from occupancy: 17 bytes * 4096 sites = 68 KiB leave two blocks of PILEUP_WAVES = 8 wavefronts per CU of the 160 KiB, four
// wavefronts per SIMD, which hides the latency of the walk's loads as the annotate kernel's three blocks do; 8192 sites would leave
// one block, two wavefronts per SIMD. A 2 kb reference is on the LDS side, a 30 kb reference is not.
#pragma once
#include <stdint.h>

#include "zsw_annotate.hpp"

namespace zsw {
namespace pile {

using ann::Rec;

constexpr int PILEUP_G = 64;                      // lanes per alignment: one wavefront
constexpr uint32_t PILEUP_WAVES = 8;              // wavefronts, i.e. alignments in flight, per block: they share the LDS accumulators
constexpr uint32_t PILEUP_LDS_SITES_MAX = 4096;   // sites whose accumulators a block keeps in LDS; beyond: every add goes to global memory

enum : int { F_READ_IS_REF = 1, F_SHARED = 2, F_CLEAR = 8, F_ALL = 11 };  // ZSW_ANNOTATE_READ_IS_REF, ZSW_ANNOTATE_SHARED, ZSW_PILEUP_CLEAR
enum : int { K_KEEP_UNCOVERED = 1, K_ALL = 1 };                            // ZSW_CONSENSUS_KEEP_UNCOVERED
enum : int { BIN_A = 0, BIN_C, BIN_G, BIN_T, BIN_N, BIN_GAP, BIN_OTHER, BIN_INVALID, N_BINS };

// The bin of a byte: A C G T/U N in either case, `-`, the other IUPAC letters in either case and `.`, everything else.
// It does not depend on the context's index_map.
ZSW_ANN_HD int bin_of(uint8_t b) {
    if (b == '-') return BIN_GAP;
    if (b == '.') return BIN_OTHER;
    const uint8_t u = (uint8_t)(b & 0xdf);  // letters: upper case
    if ((b | 0x20) < 'a' || (b | 0x20) > 'z') return BIN_INVALID;
    switch (u) {
        case 'A': return BIN_A;
        case 'C': return BIN_C;
        case 'G': return BIN_G;
        case 'T': case 'U': return BIN_T;
        case 'N': return BIN_N;
        case 'R': case 'Y': case 'S': case 'W': case 'K': case 'M': case 'B': case 'D': case 'H': case 'V': return BIN_OTHER;
        default: return BIN_INVALID;
    }
}

// The accumulators of one site: three difference arrays and the per-site misses. The workspace is len + 1 of them.
struct Diff {
    uint32_t cover, gap, skip, miss;
};
enum : int { D_COVER = 0, D_GAP = 1, D_SKIP = 2, D_MISS = 3, D_FIELDS = 4 };
// The scan that turns the difference arrays into sums over the sites in front: associative; miss is not summed.
ZSW_ANN_HD Diff combine(const Diff& a, const Diff& b) { return Diff{a.cover + b.cover, a.gap + b.gap, a.skip + b.skip, b.miss}; }

// Site `pos` of the table, given the inclusive prefix of the difference arrays up to pos and the bin of the sequence's own byte
ZSW_ANN_HD void resolve_site(uint32_t* bins, const Diff& sum, int seq_bin) {
    bins[seq_bin] += sum.cover - sum.miss;
    bins[BIN_GAP] += sum.gap;
    bins[BIN_N] += sum.skip;
}

// The first pass: may this record count? Everything is decided from the record and its ciglets; the caller has applied record_ok().
// Afterwards every site count() names lies in [0, len), every range end and insertion place in [0, len], every read byte in the read.
template <class Io>
ZSW_ANN_HD bool validate(Io& io, const Rec& a) {
    const uint64_t rlen = (uint64_t)(a.ref_end - a.ref_start), qlen = a.query_len;
    uint64_t r = 0, q = 0;  // r <= rlen and q <= qlen throughout
    for (uint32_t k = 0; k < a.n_ciglets; ++k) {
        uint32_t inc;
        uint8_t op;
        io.ciglet(k, &inc, &op);
        const int cls = ann::op_class(op);
        if (cls == ann::C_INVALID || inc == 0) return false;
        if (ann::advances_ref(cls)) {
            if ((uint64_t)inc > rlen - r) return false;
            r += inc;
        }
        if (ann::advances_query(cls)) {
            if ((uint64_t)inc > qlen - q) return false;
            q += inc;
        }
    }
    return true;
}

// The second pass over a record that passed validate(). swap: ZSW_ANNOTATE_READ_IS_REF — the record's query is the context's
// sequence and its reference the read, so I and D change places, N only moves the read cursor and S skips sites.
template <class Io>
ZSW_ANN_HD void count(Io& io, const Rec& a, bool swap, bool want_ins) {
    uint64_t r = a.ref_start, q = 0;
    for (uint32_t k = 0; k < a.n_ciglets; ++k) {
        uint32_t inc;
        uint8_t op;
        io.ciglet(k, &inc, &op);
        const int cls = ann::op_class(op);
        const uint64_t site = swap ? q : r, rd = swap ? r : q;
        const bool gap = swap ? cls == ann::C_INS : cls == ann::C_DEL, insertion = swap ? cls == ann::C_DEL : cls == ann::C_INS;
        if (cls == ann::C_COLUMN) {
            io.range(D_COVER, site, inc);
            for (uint32_t c = 0; c < inc; c += PILEUP_G) {
                const int nv = inc - c < (uint32_t)PILEUP_G ? (int)(inc - c) : PILEUP_G;
                io.columns(site + c, rd + c, nv);
            }
        } else if (gap) {
            io.range(D_GAP, site, inc);
        } else if (cls == ann::C_SKIP && !swap) {
            io.range(D_SKIP, site, inc);
        } else if (insertion && want_ins) {
            io.insertion(site, inc);
        }
        if (ann::advances_query(cls)) q += inc;
        if (ann::advances_ref(cls)) r += inc;
    }
}

// NucleotideCounts::plurality_acgtn: the largest of bins 0..4, the earlier bin on a tie (strict >), so A where nothing was counted
ZSW_ANN_HD uint8_t plurality_acgtn(const uint32_t* bins) {
    uint32_t best = bins[0];
    int at = 0;
    for (int i = 1; i < 5; ++i)
        if (bins[i] > best) {
            best = bins[i];
            at = i;
        }
    return (uint8_t)("ACGTN"[at]);
}
// ... and with K_KEEP_UNCOVERED a site without any A C G T N count keeps the caller's byte. The five bins are tested one by one:
// their 32-bit sum can wrap to zero.
ZSW_ANN_HD uint8_t consensus_byte(const uint32_t* bins, int flags, uint8_t fallback) {
    if ((flags & K_KEEP_UNCOVERED) && !(bins[0] | bins[1] | bins[2] | bins[3] | bins[4])) return fallback;
    return plurality_acgtn(bins);
}

}  // namespace pile
}  // namespace zsw
