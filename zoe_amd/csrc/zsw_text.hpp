// zsw_text.hpp — a buffer of text as arithmetic on the positions of its newlines: what the rules of zsw_fastq_parse_batch
// (zsw_fastq.hpp) and of zsw_sam_parse_batch (zsw_samtext.hpp) have in common, shared as text by the kernels (zsw_text.hip and the
// two calls' files) and the host models (tests/models/fastq_parse.cpp, samtext_parse.cpp).
//
// Three parts. (1) Newlines: the text is looked at in 16-byte granules of its ADDRESS (granule g holds the bytes at virtual
// positions 16 g .. 16 g + 15, the text's byte 0 at virtual position `head` = address & 15); a granule that lies wholly inside the
// text is one 16-byte load, the two it may share with what lies in front of and behind the text are peeled byte by byte
// (granule_words). A tile is FQ_TILE bytes of virtual positions: FQ_TILE_SWEEPS sweeps of FQ_G granules. (2) Lines: line L starts
// behind newline L - 1 and ends with newline L; chop is the readers' chop_line_break. (3) The per-byte predicates of the sweeps
// both calls make: utf8_bad_at (String::from_utf8), quality_ok.
//
// The walk is code that every lane of a group of FQ_G lanes executes with the same values; what the lanes do apart sits behind the Io:
//   io.byte(pos)                 the text's byte at pos (the caller has checked pos < n_bytes)
//   io.load16(pos, w)            the 16 bytes at pos .. pos + 15, all inside the text, their address a multiple of 16
//   io.put_position(rank, pos)   newline `rank` lies at pos
//   io.newline(rank)             the position of newline `rank` (the caller has checked rank < n_newlines)
//   io.sweep_utf8(lo, n)         true if utf8_bad_at(io, lo, n, j) for some j < n      | lane k takes j = k, k + FQ_G, ..
//   io.sweep_quality(lo, n)      true if !quality_ok(byte(lo + j)) for some j < n      |
// The kernels' Io is a wavefront (consecutive lanes, consecutive bytes, a ballot; zsw_text_dev.hpp); a model's Io loops over the lanes.
// Every position is 64-bit; nothing is narrowed. Every position taken from memory is clamped into the text before a load uses it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZSW_TEXT_HD __host__ __device__ __forceinline__
#else
#define ZSW_TEXT_HD inline
#endif

namespace zsw {
namespace text {

constexpr int FQ_G = 64;                      // lanes per record or line, and granules per sweep: one wavefront
constexpr uint32_t FQ_TILE_SWEEPS = 4;        // 16-byte loads a lane has in flight per tile
constexpr uint32_t FQ_TILE = 4096;            // bytes per tile = 16 * FQ_G * FQ_TILE_SWEEPS: one count, one wavefront
constexpr uint32_t FQ_TILE_WAVES = 4;         // tiles in flight per block of the two newline sweeps
static_assert(FQ_TILE == 16u * FQ_G * FQ_TILE_SWEEPS, "a tile is FQ_TILE_SWEEPS sweeps of FQ_G granules");

// ---- newlines ----
// 0x80 in every byte of w that is BYTE — '\n', or the byte another index is made of ('>' for zsw_fasta.hpp) (exact: no carry
// leaves a byte)
template <uint8_t BYTE = '\n'>
ZSW_TEXT_HD uint32_t nl_mask(uint32_t w) {
    const uint32_t x = w ^ (0x01010101u * BYTE);
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
ZSW_TEXT_HD uint32_t popcount32(uint32_t v) {
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}
ZSW_TEXT_HD uint64_t tiles_of(uint64_t head, uint64_t n_bytes) { return n_bytes ? (head + n_bytes + FQ_TILE - 1) / FQ_TILE : 0; }

// the four words of granule g; a byte outside the text reads as 0. head < 16.
template <class Io>
ZSW_TEXT_HD void granule_words(Io& io, uint64_t head, uint64_t n_bytes, uint64_t g, uint32_t w[4]) {
    const uint64_t v0 = g * 16u, lo = head, hi = head + n_bytes;
    if (v0 >= lo && v0 + 16u <= hi) {
        io.load16(v0 - head, w);
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
    for (uint32_t b = 0; b < 16u; ++b) {  // the head and the tail, peeled
        const uint64_t v = v0 + b;
        if (v >= lo && v < hi) w[b >> 2] |= (uint32_t)io.byte(v - head) << (8u * (b & 3u));
    }
}
template <uint8_t BYTE = '\n'>
ZSW_TEXT_HD uint32_t words_newlines(const uint32_t w[4]) {
    return popcount32(nl_mask<BYTE>(w[0]) | (nl_mask<BYTE>(w[1]) >> 1) | (nl_mask<BYTE>(w[2]) >> 2) | (nl_mask<BYTE>(w[3]) >> 3));
}
// the positions of the newlines of granule g, in order, to out[rank], out[rank + 1], .. as far as rank < cap -> how many there are
template <uint8_t BYTE = '\n', class Io>
ZSW_TEXT_HD uint32_t put_newlines(Io& io, const uint32_t w[4], uint64_t head, uint64_t g, uint64_t rank, uint64_t cap) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < 4u; ++i) {
        uint32_t m = nl_mask<BYTE>(w[i]);
        for (uint32_t b = 0; b < 4u; ++b, m >>= 8)
            if (m & 0x80u) {
                if (rank + c < cap) io.put_position(rank + c, g * 16u + 4u * i + b - head);
                ++c;
            }
    }
    return c;
}

// ---- lines ----
struct Text {
    uint64_t n_bytes, n_newlines;
    int flags;
};

// where line L starts: behind newline L - 1; n_bytes for a line the text does not have
template <class Io>
ZSW_TEXT_HD uint64_t line_start(Io& io, const Text& t, uint64_t L) {
    if (L == 0) return 0;
    if (L - 1u >= t.n_newlines) return t.n_bytes;
    const uint64_t p = io.newline(L - 1u);
    return p < t.n_bytes ? p + 1u : t.n_bytes;
}
ZSW_TEXT_HD bool line_terminated(const Text& t, uint64_t L) { return L < t.n_newlines; }

// chop_line_break on line [lo, hi): one trailing '\n' (there iff the line is terminated), then one trailing '\r' -> the new hi
template <class Io>
ZSW_TEXT_HD uint64_t chop(Io& io, uint64_t lo, uint64_t hi, bool terminated) {
    if (!terminated || hi <= lo) return hi;
    --hi;
    if (hi > lo && io.byte(hi - 1u) == '\r') --hi;
    return hi;
}

// ---- the per-byte predicates ----
ZSW_TEXT_HD bool quality_ok(uint8_t q) { return q >= '!' && q <= '~'; }
ZSW_TEXT_HD bool utf8_cont(uint8_t c) { return (c & 0xc0u) == 0x80u; }
// the bytes of the sequence a lead byte opens; 0: not a lead byte (a continuation, C0, C1, F5 .. FF)
ZSW_TEXT_HD uint32_t utf8_lead_len(uint8_t c) { return c < 0x80u ? 1u : c < 0xc2u ? 0u : c < 0xe0u ? 2u : c < 0xf0u ? 3u : c < 0xf5u ? 4u : 0u; }

// Is byte j of the header [lo, lo + n) where String::from_utf8 fails? A lead byte answers for its whole sequence (length, continuation
// bytes, overlong forms, surrogates, values above U+10FFFF); a continuation byte answers only for being covered by a lead byte in
// front of it. Some byte answers true iff the header is not UTF-8.
template <class Io>
ZSW_TEXT_HD bool utf8_bad_at(Io& io, uint64_t lo, uint64_t n, uint64_t j) {
    const uint8_t c = io.byte(lo + j);
    if (c < 0x80u) return false;
    if (utf8_cont(c)) {
        for (uint32_t d = 1; d <= 3u && d <= j; ++d) {
            const uint8_t p = io.byte(lo + j - d);
            if (!utf8_cont(p)) return utf8_lead_len(p) <= d;
        }
        return true;
    }
    const uint32_t len = utf8_lead_len(c);
    if (len == 0 || n - j < len) return true;
    const uint8_t c1 = io.byte(lo + j + 1u);
    if (!utf8_cont(c1)) return true;
    if (c == 0xe0u && c1 < 0xa0u) return true;   // overlong
    if (c == 0xedu && c1 > 0x9fu) return true;   // surrogates
    if (c == 0xf0u && c1 < 0x90u) return true;   // overlong
    if (c == 0xf4u && c1 > 0x8fu) return true;   // above U+10FFFF
    for (uint32_t k = 2; k < len; ++k)
        if (!utf8_cont(io.byte(lo + j + k))) return true;
    return false;
}

}  // namespace text
}  // namespace zsw
