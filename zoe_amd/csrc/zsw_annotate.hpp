// zsw_annotate.hpp — the rules of zsw_annotate_batch (include/zoe_sw.h), shared as text by the kernel (zsw_annotate.hip) and the
// host model (tests/models/annotate_walk.cpp): one walk of a CIGAR beside its two sequences that yields
//   sw_score_from_path (src/alignment/sw/mod.rs:399-454) with its errors in that function's own order,
//   AlignmentStates::to_verbose_sequence_matching (src/alignment/types/state.rs:320-342) through the add_state / add_ciglet merge
//   (state.rs:130-152), and the match / mismatch / gap counts.
//
// The walk is written once, as code that every lane of a group of ANN_G lanes executes with the same values ("uniform"): cursors,
// counts, the pending ciglet of the merge. What differs per lane sits behind the Io object the walk is given:
//   io.ciglet(k, &inc, &op)       ciglet k of the record
//   io.sweep(q, r, nv) -> mask    columns q + l / r + l for l < nv <= ANN_G: bit l = the two bytes match; each lane adds the weight
//                                 of its own column to a sum of its own
//   io.column_score()             the sum of those sums
//   io.emit_one(pos, inc, op)     verbose ciglet `pos` of the read, written by one lane
//   io.emit_runs(starts, mask, pos)  the runs of a sweep, one lane per run (below)
// The kernel's Io is a wavefront (one load per lane, a ballot, a reduction); the model's Io loops over the lanes.
//
// The context's sequence arrives through LDS when it is at most ANN_LDS_SEQ_MAX bytes long (a 2 kb and a 30 kb reference both are):
// 32 KiB plus 11 KiB of tables and per-wavefront buffers leave three blocks of eight wavefronts per CU of the 160 KiB, which is what
// the kernel's registers allow anyway; longer sequences are read through L2.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZSW_ANN_HD __host__ __device__ __forceinline__
#else
#define ZSW_ANN_HD inline
#endif

namespace zsw {
namespace ann {

constexpr int ANN_G = 64;                     // lanes per alignment: one wavefront
constexpr uint32_t ANN_LDS_SEQ_MAX = 32768;   // bytes of the context's sequence that are staged in LDS

// zsw_path_status
enum : uint32_t { P_OK = 0, P_REFERENCE_ENDED = 1, P_QUERY_ENDED = 2, P_FULL_QUERY_NOT_USED = 3, P_FULL_REFERENCE_NOT_USED = 4, P_INVALID_CIGAR_OP = 5,
                  P_NEGATIVE_SCORE = 6, P_NO_ALIGNMENT = 7, P_BAD_RECORD = 8 };
enum : int { F_READ_IS_REF = 1, F_SHARED = 2, F_MATCH_RESIDUES = 4, F_ALL = 7 };

// op classes: how sw_score_from_path's match arms treat an op
enum : int { C_COLUMN = 0 /* M = X */, C_INS, C_DEL, C_SOFT, C_SKIP /* N */, C_NONE /* H P */, C_INVALID };

ZSW_ANN_HD int op_class(uint8_t op) {
    switch (op) {
        case 'M': case '=': case 'X': return C_COLUMN;
        case 'I': return C_INS;
        case 'D': return C_DEL;
        case 'S': return C_SOFT;
        case 'N': return C_SKIP;
        case 'H': case 'P': return C_NONE;
        default: return C_INVALID;
    }
}
ZSW_ANN_HD bool advances_query(int cls) { return cls == C_COLUMN || cls == C_INS || cls == C_SOFT; }
ZSW_ANN_HD bool advances_ref(int cls) { return cls == C_COLUMN || cls == C_DEL || cls == C_SKIP; }
// gap_open + gap_extend * (inc - 1) with the reference's negative penalties; go / ge are the positive magnitudes, inc >= 1
ZSW_ANN_HD int64_t gap_score(int go, int ge, uint32_t inc) { return -((int64_t)go + (int64_t)ge * (int64_t)(inc - 1)); }
// A read keeps its counts and its verbose CIGAR when the walk went through every ciglet inside both sequences
ZSW_ANN_HD bool annotated(uint32_t st) { return st == P_OK || st == P_FULL_QUERY_NOT_USED || st == P_FULL_REFERENCE_NOT_USED || st == P_NEGATIVE_SCORE; }

struct Stats {  // zsw_alignment_stats
    uint32_t matches, mismatches, ins_bases, del_bases, ins_runs, del_runs;
    int32_t path_score;
    uint32_t path_status;
};

struct Rec {  // zsw_alignment
    uint32_t score, ref_start, ref_end, query_start, query_end, ref_len, query_len, n_ciglets;
    uint64_t ciglet_offset;
};

// ZSW_PATH_BAD_RECORD: ciglets outside [0, total), ranges that are no ranges, lengths that are not the sequences'.
// actual_ref / actual_query: the lengths of the sequences the flags give the record's two roles.
ZSW_ANN_HD bool record_ok(const Rec& a, uint64_t total_ciglets, uint32_t actual_ref, uint32_t actual_query) {
    if (a.ciglet_offset > total_ciglets || (uint64_t)a.n_ciglets > total_ciglets - a.ciglet_offset) return false;
    if (a.ref_start > a.ref_end || a.ref_end > a.ref_len || a.ref_len != actual_ref) return false;
    if (a.query_start > a.query_end || a.query_end > a.query_len || a.query_len != actual_query) return false;
    return true;
}

ZSW_ANN_HD int popc64(uint64_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}
ZSW_ANN_HD int ctz64(uint64_t x) {  // x != 0
#ifdef __HIP_DEVICE_COMPILE__
    return __ffsll((unsigned long long)x) - 1;
#else
    return __builtin_ctzll(x);
#endif
}
ZSW_ANN_HD int top64(uint64_t x) {  // index of the highest set bit, x != 0
#ifdef __HIP_DEVICE_COMPILE__
    return 63 - __clzll((long long)x);
#else
    return 63 - __builtin_clzll(x);
#endif
}
ZSW_ANN_HD uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// Run k of a sweep starts at bit k of `starts`; it ends in front of the next start. The last run of a sweep is not written: it
// stays pending, the next sweep or ciglet may extend it. Run k's place: pos + the starts below k.
ZSW_ANN_HD bool run_of_lane(uint64_t starts, uint64_t mask, int lane, uint32_t* inc, uint8_t* op, uint32_t* rank) {
    if (!((starts >> lane) & 1ull) || lane == top64(starts)) return false;
    const uint64_t above = starts >> (lane + 1);  // not empty: lane is not the last start
    *inc = (uint32_t)(ctz64(above) + 1);
    *op = ((mask >> lane) & 1ull) ? '=' : 'X';
    *rank = (uint32_t)popc64(starts & low_bits(lane));
    return true;
}

// The add_state / add_ciglet merge with one pending ciglet. n_out counts the ciglets that have left it.
template <bool EMIT, class Io>
struct Merge {
    int cur_op = -1;
    uint64_t cur_inc = 0;
    uint32_t n_out = 0;
    bool overflow = false;  // a merged inc beyond 32 bits

    ZSW_ANN_HD void flush(Io& io) {
        if (cur_op < 0) return;
        if (cur_inc > 0xffffffffull) overflow = true;
        if (EMIT) io.emit_one(n_out, (uint32_t)cur_inc, (uint8_t)cur_op);
        ++n_out;
        cur_op = -1;
        cur_inc = 0;
    }
    ZSW_ANN_HD void add_ciglet(Io& io, uint8_t op, uint32_t inc) {
        if (inc == 0) return;
        if ((int)op == cur_op) {
            cur_inc += inc;
            return;
        }
        flush(io);
        cur_op = op;
        cur_inc = inc;
    }
    // nv <= ANN_G calls of add_state: '=' where the bit of `mask` is set, 'X' elsewhere
    ZSW_ANN_HD void add_columns(Io& io, uint64_t mask, int nv) {
        const uint64_t valid = low_bits(nv);
        const int first_op = (mask & 1ull) ? '=' : 'X';
        uint64_t starts = ((mask ^ (mask << 1)) & valid & ~1ull) | (first_op != cur_op ? 1ull : 0ull);
        if (!starts) {
            cur_inc += (uint64_t)nv;
            return;
        }
        cur_inc += (uint64_t)ctz64(starts);  // the columns in front of the first start extend the pending ciglet
        flush(io);
        if (EMIT) io.emit_runs(starts, mask, n_out);
        const int last = top64(starts);
        n_out += (uint32_t)popc64(starts) - 1u;
        cur_op = ((mask >> last) & 1ull) ? '=' : 'X';
        cur_inc = (uint64_t)(nv - last);
    }
};

// The walk of one record that passed record_ok. Returns the stats; *n_verbose = the ciglets of the verbose CIGAR (0 for a read
// that is not annotated). ref_start is added to the reference cursor for io.sweep only.
template <bool EMIT, class Io>
ZSW_ANN_HD Stats walk(Io& io, const Rec& a, int gap_open, int gap_extend, uint32_t* n_verbose) {
    Stats s{};
    const uint64_t rlen = (uint64_t)(a.ref_end - a.ref_start), qlen = a.query_len;
    uint64_t r = 0, q = 0;
    int64_t gaps = 0;
    uint32_t err = P_OK;
    Merge<EMIT, Io> m;
    for (uint32_t k = 0; k < a.n_ciglets; ++k) {
        uint32_t inc;
        uint8_t op;
        io.ciglet(k, &inc, &op);
        const int cls = op_class(op);
        if (cls == C_INVALID) {
            err = P_INVALID_CIGAR_OP;
            break;
        }
        if (inc == 0) {  // "All increments must be nonzero" (sw/mod.rs:396-398)
            err = P_BAD_RECORD;
            break;
        }
        if (cls == C_COLUMN) {
            const uint64_t ravail = r < rlen ? rlen - r : 0, qavail = q < qlen ? qlen - q : 0;
            const uint64_t avail = ravail < qavail ? ravail : qavail;
            if ((uint64_t)inc > avail) {  // column `avail` of this ciglet: the reference is looked up first
                err = avail >= ravail ? P_REFERENCE_ENDED : P_QUERY_ENDED;
                break;
            }
            for (uint32_t c = 0; c < inc; c += ANN_G) {
                const int nv = inc - c < (uint32_t)ANN_G ? (int)(inc - c) : ANN_G;
                const uint64_t mask = io.sweep(q + c, (uint64_t)a.ref_start + r + c, nv) & low_bits(nv);
                const uint32_t eq = (uint32_t)popc64(mask);
                s.matches += eq;
                s.mismatches += (uint32_t)nv - eq;
                if (op == 'M') m.add_columns(io, mask, nv);
            }
            if (op != 'M') m.add_ciglet(io, op, inc);
        } else {
            if (cls == C_INS || cls == C_DEL) gaps += gap_score(gap_open, gap_extend, inc);
            if (cls == C_INS) {
                s.ins_bases += inc;
                ++s.ins_runs;
            }
            if (cls == C_DEL) {
                s.del_bases += inc;
                ++s.del_runs;
            }
            m.add_ciglet(io, op, inc);
        }
        if (advances_query(cls)) q += inc;
        if (advances_ref(cls)) r += inc;
    }
    m.flush(io);
    const int64_t score = io.column_score() + gaps;
    if (err == P_OK) {
        if (q < qlen) err = P_FULL_QUERY_NOT_USED;
        else if (q > qlen) err = P_QUERY_ENDED;
        else if (r < rlen) err = P_FULL_REFERENCE_NOT_USED;
        else if (r > rlen) err = P_REFERENCE_ENDED;
        else if (score < 0) err = P_NEGATIVE_SCORE;
    }
    if (annotated(err) && m.overflow) err = P_BAD_RECORD;
    if (!annotated(err)) {
        s = Stats{};
        s.path_status = err;
        *n_verbose = 0;
        return s;
    }
    s.path_status = err;
    if (err == P_OK || err == P_NEGATIVE_SCORE) s.path_score = score < -2147483647ll - 1 ? (int32_t)(-2147483647 - 1) : score > 2147483647ll ? 2147483647 : (int32_t)score;
    *n_verbose = m.n_out;
    return s;
}

}  // namespace ann
}  // namespace zsw
