// zsw_samtext.hpp — the rules of zsw_sam_parse_batch (include/zoe_sw.h), shared as text by the kernels (zsw_samtext.hip) and the host
// model (tests/models/samtext_parse.cpp): what SAMReader (src/data/records/sam/reader.rs:189-286) yields for a buffer of SAM text and
// what SamData::is_unmapped / to_alignment (sam/mod.rs:305-354) make of each data line, as arithmetic on the positions of the
// buffer's newlines. The newline index, the line bounds, chop_line_break and the UTF-8 rule are zsw_text.hpp's.
//
// Parts: (1) the Rust integer parsers (str::parse::<u16 / usize / u8 / i64>); (2) the first eleven fields of a line from ballots of
// its tabs; (3) the CIGAR: every non-digit byte's lane parses the digits in front of it (cig_lane), one uniform walk over those lanes
// in order is both iterators of cigar/iter.rs at once — CigletIterator (unchecked: ref_len_in_alignment, hence is_unmapped) and
// CigletIteratorChecked with the merge of AlignmentStates::try_from (alignment/types/std_traits.rs:119-155) — and keeps the first
// two and the last two raw ciglets for the clips; (4) the AS lookup (SamOptRaw::get + parse_value, sam/mod.rs:517-540, 581-633);
// (5) parse_line: the reader's checks in the reader's order, then the conversion.
//
// As in zsw_text.hpp every lane of a group of FQ_G lanes executes the walk with the same values; what the lanes do apart sits behind
// the Io. Beside the members zsw_text.hpp names:
//   io.mask_byte(lo, n, c)       n <= FQ_G: bit j set iff byte(lo + j) == c
//   io.sweep_byte(lo, n, c)      the lowest j < n with byte(lo + j) == c, else n
//   io.sweep_differs(lo, n)      true if byte(lo + j) != rname[j] for some j < n
//   io.cig_sweep(c_lo, lo, n)    n <= FQ_G: bit j set iff byte(lo + j) is no digit; the lane of such a byte keeps cig_lane(c_lo, lo + j)
//   io.cig_pick(j)               what lane j kept
//   io.stage(lo, hi)             the walk is about to read line [lo, hi): an Io may copy it nearer (nothing the rules depend on)
// Every position is 64-bit; every position is inside the line, which is inside the text, before a load uses it.
#pragma once
#include "zsw_text.hpp"

namespace zsw {
namespace samtext {

using namespace zsw::text;

enum : int { SF_FINAL = 1, SF_QUAL_FORWARD = 2, SF_ALL = 3 };  // ZSW_SAMTEXT_*
// the reader's errors: the first failing check of a line
enum : uint32_t { SR_OK = 0, SR_INVALID_UTF8 = 1, SR_TOO_FEW_FIELDS = 2, SR_INVALID_FLAG = 3, SR_INVALID_POS = 4, SR_INVALID_MAPQ = 5, SR_INVALID_QUALITY = 6 };
// the conversion's codes: ZSW_SAMREC_*
enum : uint32_t { SC_OK = 0, SC_SEQ_MISSING = 1, SC_CIGAR_INVALID_OP = 2, SC_CIGAR_MISSING_INC = 3, SC_CIGAR_INC_ZERO = 4, SC_CIGAR_INC_OVERFLOW = 5,
                  SC_CIGAR_MISSING_OP = 6, SC_CIGAR_MERGE_OVERFLOW = 7, SC_POS_ZERO = 8, SC_CLIPS_EXCEED_SEQ = 9, SC_TOO_LARGE = 10 };
enum : uint32_t { SB_NO_SCORE = 1, SB_OTHER_RNAME = 2, SB_SEQ_MISSING = 4, SB_QUAL_MISSING = 8, SB_QUAL_LENGTH = 16 };  // ZSW_SAMREC_BIT_*
enum : int { SI_RECORDS = 0, SI_HEADERS, SI_BASES, SI_NAME_BYTES, SI_CIGLETS, SI_CONSUMED, SI_ERROR, SI_ERROR_LINE, SI_ERROR_OFFSET, SI_MAPPED, SI_CODED,
             SI_MIN_LEN, SI_MAX_LEN, SI_WORDS };
enum : uint32_t { ST_SOME = 0, ST_UNMAPPED = 2 };  // zsw_status
enum : uint32_t { KIND_DATA = 0, KIND_HEADER = 1 };
constexpr uint32_t SAM_FIELDS = 11;
constexpr uint32_t SAM_BLOCK_LINES = 4;  // wavefronts, i.e. lines in flight, per block
constexpr uint64_t U32_MAX = 0xffffffffull;

ZSW_TEXT_HD uint64_t n_lines(const Text& t, bool last_is_newline) {
    return t.n_newlines + (((t.flags & SF_FINAL) && t.n_bytes && !last_is_newline) ? 1u : 0u);
}
ZSW_TEXT_HD uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
ZSW_TEXT_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
ZSW_TEXT_HD bool is_ascii_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\x0c' || c == '\r'; }  // u8::is_ascii_whitespace
ZSW_TEXT_HD bool is_cigar_op(uint8_t c) {
    return c == 'M' || c == 'I' || c == 'D' || c == 'N' || c == 'S' || c == 'H' || c == 'P' || c == 'X' || c == '=';
}
ZSW_TEXT_HD bool op_takes_ref(uint8_t c) { return c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X'; }

// ---- the integer parsers ----
// str::parse for an unsigned type with the largest value `max`: one optional '+', then at least one digit and nothing else
template <class Io>
ZSW_TEXT_HD bool parse_unsigned(Io& io, uint64_t lo, uint64_t n, uint64_t max, uint64_t* out) {
    uint64_t j = (n && io.byte(lo) == '+') ? 1u : 0u, x = 0;
    if (j == n) return false;
    for (; j < n; ++j) {
        const uint8_t c = io.byte(lo + j);
        if (!is_digit(c)) return false;
        const uint64_t d = c - '0';
        if (x > (max - d) / 10u) return false;
        x = x * 10u + d;
    }
    *out = x;
    return true;
}
// str::parse::<i64> narrowed to what the score takes: true iff the value parses AND lies in 0 ..= 2^32 - 1 ("-0" is 0)
template <class Io>
ZSW_TEXT_HD bool parse_score(Io& io, uint64_t lo, uint64_t n, uint32_t* out) {
    uint64_t x = 0;
    if (n && io.byte(lo) == '-') {
        if (n == 1u) return false;
        for (uint64_t j = 1; j < n; ++j)
            if (io.byte(lo + j) != '0') return false;  // a negative value, or no number
    } else if (!parse_unsigned(io, lo, n, U32_MAX, &x))
        return false;
    *out = (uint32_t)x;
    return true;
}

// ---- fields ----
// The first eleven fields of line [lo, hi): field k is [f[k], e[k]). -> how many there are (at most eleven); *more: an eleventh tab
// ends field 10 and optional fields start behind it.
template <class Io>
ZSW_TEXT_HD uint32_t split_fields(Io& io, uint64_t lo, uint64_t hi, uint64_t f[SAM_FIELDS], uint64_t e[SAM_FIELDS], bool* more) {
    uint32_t k = 0;
    const uint64_t n = hi - lo;
    f[0] = lo;
    for (uint64_t j0 = 0; j0 < n && k < SAM_FIELDS; j0 += FQ_G) {
        uint64_t m = io.mask_byte(lo + j0, n - j0 < (uint64_t)FQ_G ? n - j0 : (uint64_t)FQ_G, '\t');
        while (m && k < SAM_FIELDS) {
            e[k] = lo + j0 + (uint64_t)__builtin_ctzll(m);
            m &= m - 1u;
            ++k;
            if (k < SAM_FIELDS) f[k] = e[k - 1] + 1u;
        }
    }
    *more = k == SAM_FIELDS;
    if (k < SAM_FIELDS) e[k++] = hi;
    return k;
}

// ---- the CIGAR ----
enum : uint32_t { CL_OVERFLOW = 0x100, CL_NO_DIGITS = 0x200, CL_BAD_OP = 0x400 };
struct CigLane {
    uint64_t inc;
    uint32_t bits;  // the byte, CL_*
};
// what the lane of the non-digit byte at p finds: the digits in front of it back to the CIGAR's start or the non-digit before them
template <class Io>
ZSW_TEXT_HD CigLane cig_lane(Io& io, uint64_t c_lo, uint64_t p) {
    uint64_t s = p;
    while (s > c_lo && is_digit(io.byte(s - 1u))) --s;
    CigLane L{0, io.byte(p)};
    if (s == p) L.bits |= CL_NO_DIGITS;
    if (!is_cigar_op((uint8_t)L.bits)) L.bits |= CL_BAD_OP;
    for (uint64_t q = s; q < p; ++q) {
        const uint64_t d = io.byte(q) - '0';
        if (L.inc > (~0ull - d) / 10u) {
            L.bits |= CL_OVERFLOW;
            break;
        }
        L.inc = L.inc * 10u + d;
    }
    return L;
}

struct Raw {
    uint64_t inc;
    uint32_t op;
};
struct Cigar {
    uint32_t err;            // the first error of CigletIteratorChecked (SC_CIGAR_INVALID_OP .. SC_CIGAR_MISSING_OP), 0: none
    bool merge_overflow;     // a merged inc left 64 bits
    bool wide;               // a merged inc beyond 32 bits
    uint64_t ref_len;        // the sum of inc over M D N = X that the unchecked iterator yields, saturating
    uint64_t n_raw;          // raw ciglets in front of the first error
    Raw first0, first1;      // raw ciglets 0 and 1            | four values, not two arrays: an index that is not a constant
    Raw last0, last1;        // raw ciglets n_raw - 1, n_raw - 2 | would put the struct into scratch memory on the device
    uint64_t n_merged;       // ciglets after the merge (meaningful without an error)
};
struct NoSink {
    ZSW_TEXT_HD void put(uint64_t, uint64_t, uint32_t) const {}
};

// One walk over the CIGAR [c_lo, c_hi); sink.put(k, inc, op) receives merged ciglet k as soon as it is complete.
template <class Io, class Sink>
ZSW_TEXT_HD Cigar walk_cigar(Io& io, uint64_t c_lo, uint64_t c_hi, Sink& sink) {
    Cigar C{};
    const uint64_t n = c_hi - c_lo;
    uint64_t cur_inc = 0, tail = c_lo;  // tail: one behind the last non-digit
    uint32_t cur_op = 0;
    bool stopped = false;               // the unchecked iterator has ended
    for (uint64_t j0 = 0; j0 < n && !stopped; j0 += FQ_G) {
        uint64_t m = io.cig_sweep(c_lo, c_lo + j0, n - j0 < (uint64_t)FQ_G ? n - j0 : (uint64_t)FQ_G);
        while (m) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            m &= m - 1u;
            const CigLane L = io.cig_pick(b);
            const uint32_t op = L.bits & 0xffu;
            tail = c_lo + j0 + b + 1u;
            // the order of the byte positions: the digit that overflows lies in front of the op, the op is where the other three show
            const uint32_t e = (L.bits & CL_OVERFLOW) ? SC_CIGAR_INC_OVERFLOW : (L.bits & CL_BAD_OP) ? SC_CIGAR_INVALID_OP : (L.bits & CL_NO_DIGITS) ? SC_CIGAR_MISSING_INC
                               : L.inc == 0 ? SC_CIGAR_INC_ZERO : 0u;
            if (e && !C.err) C.err = e;
            if (L.bits & (CL_OVERFLOW | CL_BAD_OP | CL_NO_DIGITS)) {
                stopped = true;
                break;
            }
            if (op_takes_ref((uint8_t)op)) C.ref_len = sat_add(C.ref_len, L.inc);
            if (C.err) continue;  // only the unchecked iterator goes on (behind an inc of 0)
            if (C.n_raw == 0) C.first0 = Raw{L.inc, op};
            if (C.n_raw == 1u) C.first1 = Raw{L.inc, op};
            C.last1 = C.last0;
            C.last0 = Raw{L.inc, op};
            ++C.n_raw;
            if (op == cur_op) {
                if (cur_inc + L.inc < cur_inc) C.merge_overflow = true;
                cur_inc += L.inc;
            } else {
                if (cur_op) {
                    if (cur_inc > U32_MAX) C.wide = true;
                    sink.put(C.n_merged++, cur_inc, cur_op);
                }
                cur_op = op;
                cur_inc = L.inc;
            }
        }
    }
    if (!stopped && tail < c_hi && !C.err) {  // digits without an op behind them: the checked iterator alone minds
        uint64_t x = 0;
        C.err = SC_CIGAR_MISSING_OP;
        for (uint64_t q = tail; q < c_hi; ++q) {
            const uint64_t d = io.byte(q) - '0';
            if (x > (~0ull - d) / 10u) {
                C.err = SC_CIGAR_INC_OVERFLOW;
                break;
            }
            x = x * 10u + d;
        }
    }
    if (cur_op && !C.err) {
        if (cur_inc > U32_MAX) C.wide = true;
        sink.put(C.n_merged++, cur_inc, cur_op);
    }
    return C;
}

// to_alignment's clips on the raw ciglets: from the front one optional H, then one optional S; from the back the same among the rest
ZSW_TEXT_HD void soft_clips(const Cigar& C, uint64_t* front, uint64_t* back) {
    uint64_t i = 0, j = C.n_raw;
    *front = *back = 0;
    if (i < j && C.first0.op == 'H') ++i;
    if (i < j) {
        const Raw r = i ? C.first1 : C.first0;
        if (r.op == 'S') {
            *front = r.inc;
            ++i;
        }
    }
    if (j > i && C.last0.op == 'H') --j;
    if (j > i) {
        const Raw r = j == C.n_raw ? C.last0 : C.last1;
        if (r.op == 'S') *back = r.inc;
    }
}

// ---- AS ----
// opt_fields.get("AS") then .int() over the optional fields [lo, hi): true and the score iff Ok(Some(v)) with 0 <= v <= 2^32 - 1
template <class Io>
ZSW_TEXT_HD bool find_score(Io& io, uint64_t lo, uint64_t hi, uint32_t* score) {
    for (;;) {
        const uint64_t f_hi = lo + io.sweep_byte(lo, hi - lo, '\t');
        const uint64_t c1 = io.sweep_byte(lo, f_hi - lo, ':');
        if (lo + c1 == f_hi) return false;  // Err: a field without a colon
        if (c1 == 2u && io.byte(lo) == 'A' && io.byte(lo + 1u) == 'S') {
            const uint64_t t_lo = lo + 3u;
            const uint64_t c2 = io.sweep_byte(t_lo, f_hi - t_lo, ':');
            if (t_lo + c2 == f_hi) return false;
            if (c2 != 1u || io.byte(t_lo) != 'i') return false;  // no type, another type, or more than one character
            return parse_score(io, t_lo + 2u, f_hi - (t_lo + 2u), score);
        }
        if (f_hi == hi) return false;  // Ok(None)
        lo = f_hi + 1u;
    }
}

// ---- one line ----
struct Line {
    uint64_t name_lo, name_len, seq_lo, seq_len, qual_lo, cig_lo, cig_len, pos;
    uint32_t kind, code, rec_code, bits, status, n_ciglets, flag, mapq;
    uint32_t qual_fill;  // the qualities are '!' (QUAL missing or of another length)
    uint32_t score, ref_start, ref_end, query_start, query_end;
};

// rname_len == 0: no RNAME to compare with
template <class Io>
ZSW_TEXT_HD Line parse_line(Io& io, const Text& t, uint64_t L, uint32_t rname_len) {
    Line R{};
    const uint64_t lo = line_start(io, t, L);
    uint64_t hi = line_start(io, t, L + 1u);
    if (hi < lo) hi = lo;
    io.stage(lo, hi);
    hi = chop(io, lo, hi, line_terminated(t, L));
    R.name_lo = R.seq_lo = R.qual_lo = R.cig_lo = lo;
    if (io.sweep_utf8(lo, hi - lo)) {
        R.code = SR_INVALID_UTF8;
        return R;
    }
    if (hi > lo && io.byte(lo) == '@') {
        R.kind = KIND_HEADER;
        return R;
    }
    uint64_t f[SAM_FIELDS], e[SAM_FIELDS], v = 0;
    bool more = false;
    if (split_fields(io, lo, hi, f, e, &more) < SAM_FIELDS) {
        R.code = SR_TOO_FEW_FIELDS;
        return R;
    }
    if (!parse_unsigned(io, f[1], e[1] - f[1], 0xffffull, &v)) {
        R.code = SR_INVALID_FLAG;
        return R;
    }
    R.flag = (uint32_t)v;
    if (!parse_unsigned(io, f[3], e[3] - f[3], ~0ull, &R.pos)) {
        R.code = SR_INVALID_POS;
        return R;
    }
    if (!parse_unsigned(io, f[4], e[4] - f[4], 0xffull, &v)) {
        R.code = SR_INVALID_MAPQ;
        return R;
    }
    R.mapq = (uint32_t)v;
    const uint64_t q_len = e[10] - f[10];
    const bool qual_missing = q_len == 0 || (q_len == 1u && io.byte(f[10]) == '*');
    if (!qual_missing && io.sweep_quality(f[10], q_len)) {
        R.code = SR_INVALID_QUALITY;
        return R;
    }
    // the record
    R.name_lo = f[0];
    R.name_len = e[0] - f[0];
    const uint64_t s_len = e[9] - f[9];
    const bool seq_missing = s_len == 0 || (s_len == 1u && io.byte(f[9]) == '*');
    R.seq_lo = f[9];
    R.seq_len = seq_missing ? 0 : s_len;
    R.qual_lo = f[10];
    if (seq_missing) R.bits |= SB_SEQ_MISSING;
    if (qual_missing) R.bits |= SB_QUAL_MISSING;
    else if (q_len != R.seq_len) R.bits |= SB_QUAL_LENGTH;
    R.qual_fill = (R.bits & (SB_QUAL_MISSING | SB_QUAL_LENGTH)) ? 1u : 0u;
    if (!more || !find_score(io, e[10] + 1u, hi, &R.score)) {
        R.score = 0;
        R.bits |= SB_NO_SCORE;
    }
    uint64_t c_lo = f[5], c_hi = e[5];  // trim_ascii; "*" is the empty CIGAR
    while (c_lo < c_hi && is_ascii_space(io.byte(c_lo))) ++c_lo;
    while (c_hi > c_lo && is_ascii_space(io.byte(c_hi - 1u))) --c_hi;
    if (c_hi - c_lo == 1u && io.byte(c_lo) == '*') c_hi = c_lo;
    R.cig_lo = c_lo;
    R.cig_len = c_hi - c_lo;
    NoSink none;
    const Cigar C = walk_cigar(io, c_lo, c_hi, none);
    R.status = ST_UNMAPPED;
    const uint32_t score = R.score;
    R.score = 0;
    if ((R.flag & 4u) || C.ref_len == 0) return R;  // is_unmapped
    if (rname_len && (e[2] - f[2] != rname_len || io.sweep_differs(f[2], rname_len))) {
        R.bits |= SB_OTHER_RNAME;
        return R;
    }
    uint64_t front, back;
    soft_clips(C, &front, &back);
    const uint64_t ref_end = sat_add(R.pos - 1u, C.ref_len);
    if (seq_missing) R.rec_code = SC_SEQ_MISSING;
    else if (C.err) R.rec_code = C.err;
    else if (C.merge_overflow) R.rec_code = SC_CIGAR_MERGE_OVERFLOW;
    else if (R.pos == 0) R.rec_code = SC_POS_ZERO;
    else if (sat_add(front, back) > R.seq_len) R.rec_code = SC_CLIPS_EXCEED_SEQ;
    else if (C.wide || ref_end > U32_MAX || R.seq_len > U32_MAX || C.n_merged > U32_MAX) R.rec_code = SC_TOO_LARGE;
    if (R.rec_code) return R;
    R.status = ST_SOME;
    R.score = score;
    R.ref_start = (uint32_t)(R.pos - 1u);
    R.ref_end = (uint32_t)ref_end;
    R.query_start = (uint32_t)front;
    R.query_end = (uint32_t)(R.seq_len - back);
    R.n_ciglets = (uint32_t)C.n_merged;
    return R;
}

}  // namespace samtext
}  // namespace zsw
