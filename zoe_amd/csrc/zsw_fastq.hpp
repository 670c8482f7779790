// zsw_fastq.hpp — the rules of zsw_fastq_parse_batch (include/zoe_sw.h), shared as text by the kernels (zsw_fastq.hip) and the
// host model (tests/models/fastq_parse.cpp): what FastQReader (src/data/records/fastq/reader.rs:87-187) yields for a buffer of
// single-line FASTQ, as arithmetic on the positions of the buffer's newlines.
//
// The newlines, the line bounds, chop_line_break, the UTF-8 rule and quality_ok are zsw_text.hpp's. This header adds the records:
// record r is lines 4 r .. 4 r + 3 (record_bounds: five positions); parse_record makes the reader's checks in the reader's order
// and says where name, bases and qualities lie. Beside the members of the Io that zsw_text.hpp names:
//   io.sweep_blank(lo, n)        the lowest j < n with is_blank(byte(lo + j)), else n  | lane k takes j = k, k + FQ_G, ..
#pragma once
#include "zsw_text.hpp"

namespace zsw {
namespace fastq {

using namespace zsw::text;

constexpr uint32_t FQ_BLOCK_RECORDS = 8;      // wavefronts, i.e. records in flight, per block

// The shapes this header's walk and its tests are written for (the tests read them from this file), held to zsw_text.hpp's
namespace shapes { constexpr int FQ_G = 64; constexpr uint32_t FQ_TILE_SWEEPS = 4; constexpr uint32_t FQ_TILE = 4096; }
static_assert(shapes::FQ_G == text::FQ_G && shapes::FQ_TILE_SWEEPS == text::FQ_TILE_SWEEPS && shapes::FQ_TILE == text::FQ_TILE, "zsw_text.hpp has other shapes");

enum : int { F_FINAL = 1, F_NAME_TO_BLANK = 2, F_ALL = 3 };  // ZSW_FASTQ_*
enum : uint32_t { OK = 0, MISSING_AT = 1, MISSING_HEADER = 2, INVALID_UTF8 = 3, MISSING_SEQUENCE = 4, MISSING_PLUS = 5, MISSING_QUALITY = 6,
                  LENGTH_MISMATCH = 7, INVALID_QUALITY = 8 };
enum : int { INFO_RECORDS = 0, INFO_BASES, INFO_NAME_BYTES, INFO_CONSUMED, INFO_ERROR, INFO_ERROR_RECORD, INFO_ERROR_OFFSET, INFO_MIN_LEN, INFO_MAX_LEN,
             INFO_WORDS };

// the records the call parses; last_is_newline: text[n_bytes - 1] == '\n' (anything for an empty text)
ZSW_TEXT_HD uint64_t n_records(const Text& t, bool last_is_newline) {
    if (!(t.flags & F_FINAL)) return t.n_newlines / 4u;
    const uint64_t lines = t.n_newlines + ((t.n_bytes && !last_is_newline) ? 1u : 0u);
    return lines / 4u + ((lines & 3u) ? 1u : 0u);
}

// b[k] = the start of line 4 r + k, k = 0 .. 4, never descending: line k of the record is [b[k], b[k + 1]), its newline included
template <class Io>
ZSW_TEXT_HD void record_bounds(Io& io, const Text& t, uint64_t r, uint64_t b[5]) {
    for (uint32_t k = 0; k < 5u; ++k) {
        b[k] = line_start(io, t, 4u * r + k);
        if (k && b[k] < b[k - 1]) b[k] = b[k - 1];
    }
}

ZSW_TEXT_HD bool is_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// ---- one record ----
struct Record {
    uint32_t code;                 // 0, or the first failing check
    uint64_t name_lo, name_len;    // the name (the header behind '@', chopped; with F_NAME_TO_BLANK up to the first blank)
    uint64_t seq_lo, seq_len;      // bases; the qualities are seq_len bytes at qual_lo
    uint64_t qual_lo;
};

// where the parts of record r lie, without a check (the gather: the record pass has found the record good)
template <class Io>
ZSW_TEXT_HD Record locate_record(Io& io, const Text& t, uint64_t r) {
    uint64_t b[5];
    record_bounds(io, t, r, b);
    Record R{};
    R.name_lo = b[0] < b[1] ? b[0] + 1u : b[0];
    R.seq_lo = b[1];
    R.qual_lo = b[3];
    return R;
}

// the reader's checks, in the reader's order
template <class Io>
ZSW_TEXT_HD Record parse_record(Io& io, const Text& t, uint64_t r) {
    uint64_t b[5];
    record_bounds(io, t, r, b);
    Record R{};
    R.name_lo = b[0];
    R.seq_lo = b[1];
    R.qual_lo = b[3];
    if (b[1] == b[0] || io.byte(b[0]) != '@') {
        R.code = MISSING_AT;
        return R;
    }
    R.name_lo = b[0] + 1u;
    const uint64_t h_hi = chop(io, R.name_lo, b[1], line_terminated(t, 4u * r));
    const uint64_t h_len = h_hi - R.name_lo;
    if (h_len == 0) {
        R.code = MISSING_HEADER;
        return R;
    }
    if (io.sweep_utf8(R.name_lo, h_len)) {
        R.code = INVALID_UTF8;
        return R;
    }
    R.name_len = (t.flags & F_NAME_TO_BLANK) ? io.sweep_blank(R.name_lo, h_len) : h_len;
    R.seq_len = chop(io, b[1], b[2], line_terminated(t, 4u * r + 1u)) - b[1];
    if (R.seq_len == 0) {
        R.code = MISSING_SEQUENCE;
        return R;
    }
    if (b[3] == b[2] || io.byte(b[2]) != '+') {
        R.code = MISSING_PLUS;
        return R;
    }
    const uint64_t q_len = chop(io, b[3], b[4], line_terminated(t, 4u * r + 3u)) - b[3];
    if (q_len == 0) {
        R.code = MISSING_QUALITY;
        return R;
    }
    if (q_len != R.seq_len) {
        R.code = LENGTH_MISMATCH;
        return R;
    }
    if (io.sweep_quality(b[3], q_len)) R.code = INVALID_QUALITY;
    return R;
}

}  // namespace fastq
}  // namespace zsw
