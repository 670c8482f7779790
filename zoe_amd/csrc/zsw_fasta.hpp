// zsw_fasta.hpp — the rules of zsw_fasta_parse_batch (include/zoe_sw.h), shared as text by the kernels (zsw_fasta.hip) and the
// host model (tests/models/fasta_parse.cpp): what FastaReader (src/data/records/fasta/mod.rs:241-410) yields for a buffer of FASTA,
// as arithmetic on the positions of the buffer's '>' bytes.
//
// The granules, the tiles and the index are zsw_text.hpp's, made over '>' instead of '\n' (Text::n_newlines counts the '>' here).
// Every '>' delimits: record r is the region behind '>' r up to '>' r + 1 or the end of the text. This header adds
//   check_start     the reader's start of the file: whitespace lines, then a '>' at a line start
//   parse_record    one record, the reader's checks in the reader's order: where the header ends, where the body starts, the name,
//                   and EVERY code — also MISSING_SEQUENCE: the pass looks past the line breaks that open the body for the first byte
//                   that stays. That costs a walk over a run of line breaks, no more than the header walk costs over a header, and it
//                   is what the reader's own quirk asks for anyway (a later record without a sequence byte is MISSING_SEQUENCE or
//                   GT_IN_HEADER by whether its region holds a '\n'). In return the lowest failing record is known before the sequence
//                   pass, which is then a plain compaction with one cut.
//   granule_bases   the sequence pass for one granule: a byte stays if it lies in the body of its record, in front of the cut (the '>'
//                   of the first record that is not delivered) and is neither '\n' nor '\r'; its record is the number of '>' in front
//                   of it. Counted in one sweep, written at its rank in the next; the lane that meets '>' r writes offset r.
// Beside the members of the Io that zsw_text.hpp names:
//   io.sweep_class(lo, n, cls)        the lowest j < n with in_class(byte(lo + j), cls), else n   | lane k takes j = k, k + FQ_G, ..
//   io.sweep_class_last(lo, n, cls)   the highest such j, else n                                  |
//   io.body_lo(r)                     where the body of record r starts (the record pass wrote it)
//   io.put_base(rank, c)              byte c is base `rank` of the output
//   io.put_offset(r, kept)            `kept` bases lie in front of record r
#pragma once
#include "zsw_text.hpp"

namespace zsw {
namespace fasta {

using namespace zsw::text;

constexpr uint32_t FA_BLOCK_RECORDS = 8;      // wavefronts, i.e. records in flight, per block of the record pass and the gather

enum : int { F_FINAL = 1, F_NAME_TO_BLANK = 2, F_CONTINUED = 4, F_ALL = 7 };  // ZSW_FASTA_*
enum : uint32_t { OK = 0, NO_DATA = 1, MISSING_GT = 2, MISSING_HEADER = 3, GT_IN_HEADER = 4, MISSING_SEQUENCE = 5, GT_IN_SEQUENCE = 6 };
enum : int { INFO_RECORDS = 0, INFO_BASES, INFO_NAME_BYTES, INFO_CONSUMED, INFO_ERROR, INFO_ERROR_RECORD, INFO_ERROR_OFFSET, INFO_MIN_LEN, INFO_MAX_LEN,
             INFO_WORDS };

enum : int { C_NEWLINE = 0, C_BREAK, C_NOT_BREAK, C_NOT_SPACE, C_BLANK };
// u8::is_ascii_whitespace: '\x0b' is none
ZSW_TEXT_HD bool is_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\x0c' || c == '\r'; }
ZSW_TEXT_HD bool is_break(uint8_t c) { return c == '\n' || c == '\r'; }
ZSW_TEXT_HD bool in_class(uint8_t c, int cls) {
    return cls == C_NEWLINE ? c == '\n' : cls == C_BREAK ? is_break(c) : cls == C_NOT_BREAK ? !is_break(c) : cls == C_NOT_SPACE ? !is_space(c) : (c == ' ' || c == '\t');
}

// the records the call parses out of n_gt regions: without FINAL the last region may go on in the next buffer
ZSW_TEXT_HD uint64_t n_records(const Text& t, bool) { return (t.flags & F_FINAL) ? t.n_newlines : (t.n_newlines ? t.n_newlines - 1u : 0u); }

// where '>' r lies, clamped into the text; n_bytes for one the text does not have
template <class Io>
ZSW_TEXT_HD uint64_t gt_at(Io& io, const Text& t, uint64_t r) {
    if (r >= t.n_newlines) return t.n_bytes;
    const uint64_t p = io.newline(r);
    return p < t.n_bytes ? p : t.n_bytes;
}

// ---- the start of the file (not with F_CONTINUED) ----
struct Start {
    uint32_t code;      // 0, NO_DATA or MISSING_GT
    uint64_t offset;    // MISSING_GT: the first byte that is not whitespace
    uint64_t consumed;  // a text without '>': behind its last terminated line
};
// Lines that are all whitespace are skipped; the first other line starts with '>'. In positions: nothing but whitespace in front of
// the first '>', and that '>' at the start of the text or behind a '\n'.
template <class Io>
ZSW_TEXT_HD Start check_start(Io& io, const Text& t) {
    Start s{};
    const uint64_t g0 = gt_at(io, t, 0);
    const uint64_t p = io.sweep_class(0, g0, C_NOT_SPACE);
    if (p < g0 || (g0 < t.n_bytes && g0 > 0 && io.byte(g0 - 1u) != '\n')) {
        s.code = MISSING_GT;
        s.offset = p;  // p == g0: the '>' itself, which does not start its line
        return s;
    }
    if (g0 == t.n_bytes) {  // whitespace and nothing else
        if (t.flags & F_FINAL) {
            s.code = NO_DATA;
            return s;
        }
        const uint64_t last = io.sweep_class_last(0, t.n_bytes, C_NEWLINE);
        s.consumed = last < t.n_bytes ? last + 1u : 0u;
    }
    return s;
}

// ---- one record ----
struct Record {
    uint32_t code;               // 0, or the first failing check
    uint64_t name_lo, name_len;  // the name (the header; with F_NAME_TO_BLANK up to the first blank)
    uint64_t body_lo;            // the region behind the header's line break: the bytes of it that are no line break are the sequence
};

template <class Io>
ZSW_TEXT_HD Record parse_record(Io& io, const Text& t, uint64_t r) {
    Record R{};
    const uint64_t s = gt_at(io, t, r) + 1u;  // r < n_records: '>' r is there, s <= n_bytes
    const bool has_gt = r + 1u < t.n_newlines;
    uint64_t e = gt_at(io, t, r + 1u);
    if (e < s) e = s;  // positions from memory: never descending
    R.name_lo = s;
    R.body_lo = e;
    uint64_t h_hi;
    bool header_newline;  // the header's line break is a '\n'
    if (r == 0 && !(t.flags & F_CONTINUED)) {
        // read_first_record: the header is the line, chopped (one '\n', then one '\r'); a '\r' inside it stays
        const uint64_t nl = s + io.sweep_class(s, e - s, C_NEWLINE);
        if (nl == e) {
            if (has_gt) {  // the line holds the next '>'
                R.code = GT_IN_HEADER;
                return R;
            }
            R.code = s == e ? MISSING_HEADER : MISSING_SEQUENCE;  // an unterminated header ends the file
            return R;
        }
        h_hi = nl;
        if (h_hi > s && io.byte(h_hi - 1u) == '\r') --h_hi;
        if (h_hi == s) {
            R.code = MISSING_HEADER;
            return R;
        }
        R.body_lo = nl + 1u;
        header_newline = true;
    } else {
        // next: the region is split at every '\n' and '\r'; its first piece is the name
        if (s == e) {  // ">>": the piece is the '>' itself, not empty, and nothing follows it
            R.code = has_gt ? GT_IN_HEADER : MISSING_HEADER;
            return R;
        }
        const uint64_t lb = s + io.sweep_class(s, e - s, C_BREAK);
        if (lb == e) {  // no line break: no sequence; the reader reads on to the end of the line to name the header
            R.code = has_gt ? GT_IN_HEADER : MISSING_SEQUENCE;
            return R;
        }
        if (lb == s) {
            R.code = MISSING_HEADER;
            return R;
        }
        h_hi = lb;
        R.body_lo = lb + 1u;
        header_newline = io.byte(lb) == '\n';
    }
    const uint64_t h_len = h_hi - s;
    R.name_len = (t.flags & F_NAME_TO_BLANK) ? io.sweep_class(s, h_len, C_BLANK) : h_len;
    const uint64_t b_len = e - R.body_lo;
    if (io.sweep_class(R.body_lo, b_len, C_NOT_BREAK) == b_len) {  // no byte of the body stays
        R.code = MISSING_SEQUENCE;
        // a later record that ends at '>': the reader asks whether it has read a whole line, i.e. whether the region holds a '\n'
        if (!(r == 0 && !(t.flags & F_CONTINUED)) && has_gt && !header_newline && io.sweep_class(R.body_lo, b_len, C_NEWLINE) == b_len) R.code = GT_IN_HEADER;
        return R;
    }
    if (has_gt && io.byte(e - 1u) != '\n') R.code = GT_IN_SEQUENCE;  // the body is not empty: e - 1 >= body_lo
    return R;
}

// where the name of record r starts, without a check (the gather: the record pass has found the record good)
template <class Io>
ZSW_TEXT_HD uint64_t name_start(Io& io, const Text& t, uint64_t r) { return gt_at(io, t, r) + 1u; }

// ---- the sequence pass ----
// Granule g (words w, bytes outside the text read as 0 and are skipped), n_gt_front '>' in front of it, `rank` kept bytes in front of
// it (WRITE only) -> the bytes of the granule that stay. n_body: the records whose body_lo the record pass wrote. WRITE: every kept
// byte to its rank, and the offset of every record whose '>' lies here.
template <bool WRITE, class Io>
ZSW_TEXT_HD uint32_t granule_bases(Io& io, const uint32_t w[4], uint64_t head, uint64_t n_bytes, uint64_t g, uint64_t n_gt_front, uint64_t n_body, uint64_t cut,
                                   uint64_t rank) {
    const uint64_t v0 = g * 16u;
    if (v0 >= head + n_bytes || v0 + 16u <= head) return 0;
    if (v0 >= head && v0 - head > cut) return 0;  // behind the cut nothing stays and no offset is asked for
    uint64_t lo = (n_gt_front && n_gt_front - 1u < n_body) ? io.body_lo(n_gt_front - 1u) : ~0ull;
    uint32_t kept = 0;
    for (uint32_t b = 0; b < 16u; ++b) {
        const uint64_t v = v0 + b;
        if (v < head || v >= head + n_bytes) continue;
        const uint64_t p = v - head;
        const uint8_t c = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
        if (c == '>') {
            if (WRITE) io.put_offset(n_gt_front, rank + kept);
            lo = n_gt_front < n_body ? io.body_lo(n_gt_front) : ~0ull;
            ++n_gt_front;
            continue;
        }
        if (p >= lo && p < cut && !is_break(c)) {
            if (WRITE) io.put_base(rank + kept, c);
            ++kept;
        }
    }
    return kept;
}

}  // namespace fasta
}  // namespace zsw
