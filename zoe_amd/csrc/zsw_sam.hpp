// zsw_sam.hpp — the rules of zsw_sam_batch (include/zoe_sw.h), shared as text by the kernel (zsw_sam.hip) and the host model
// (tests/models/sam_line.cpp): what SamData::from_alignment (src/data/records/sam/mod.rs:223-245) followed by Display for SamData
// (records/sam/std_traits.rs:3-44) print for one read, as a layout — which byte of the line is which byte of which field.
//
// One function, line<WRITE>(), walks the fields of a line in their order. With WRITE = false it only adds up their lengths: that
// is line_length(), what the length launch stores per read. With WRITE = true the same walk hands every field to an Io object at
// the place the walk has reached: that is write_line(), the write launch. Both launches get lengths and places from this one
// walk, so the bytes a read was given by the scan and the bytes its write lays down cannot disagree.
//
// The walk is code that every lane of a group of SAM_G lanes executes with the same values ("uniform"); what the lanes do apart
// sits behind the Io:
//   io.put8(pos, w, n)                 bytes pos .. pos + n - 1 (n <= 8) = the low n bytes of w, lowest first
//   io.name / rname / seq (pos, n)     n bytes of the read's QNAME / of RNAME / of the read's bases, copied
//   io.qual(pos, n, reversed)          n quality bytes, back to front if reversed
//   io.cigar_sweep<WRITE>(pos, k0, nv, &bad) -> chars
//                                      ciglets k0 .. k0 + nv - 1 (nv <= SAM_G) of the record, lane k takes ciglet k0 + k: the
//                                      characters they take together (ciglet_chars), *bad set if one is not ciglet_ok; WRITE:
//                                      each one written by put_ciglet at pos + the characters of the ciglets in front of it
//   io.put_lane(pos, byte)             one byte, by the lane that calls it (put_ciglet)
// The kernel's Io is a wavefront (consecutive lanes, consecutive bytes; a prefix sum across the lanes); the model's Io loops.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZSW_SAM_HD __host__ __device__ __forceinline__
#else
#define ZSW_SAM_HD inline
#endif

namespace zsw {
namespace sam {

constexpr int SAM_G = 64;                    // lanes per line: one wavefront
constexpr uint32_t SAM_BLOCK_LINES = 8;      // wavefronts, i.e. lines in flight, per block
constexpr uint32_t SAM_LDS_LINE = 1024;      // bytes of a line that are assembled in LDS (longer lines: written straight to memory)

enum : int { F_OMIT_SEQ = 1, F_ALL = 1 };    // ZSW_SAM_*
constexpr uint8_t STATUS_SOME = 0;           // ZSW_STATUS_SOME

struct Rec {  // zsw_alignment
    uint32_t score, ref_start, ref_end, query_start, query_end, ref_len, query_len, n_ciglets;
    uint64_t ciglet_offset;
};

// the record's ciglets lie inside [0, total): 64-bit, before any ciglet load
ZSW_SAM_HD bool ciglets_in_range(const Rec& a, uint64_t total_ciglets) {
    return a.ciglet_offset <= total_ciglets && (uint64_t)a.n_ciglets <= total_ciglets - a.ciglet_offset;
}

ZSW_SAM_HD bool op_ok(uint8_t op) {
    switch (op) {
        case 'M': case 'I': case 'D': case 'N': case 'S': case 'H': case 'P': case '=': case 'X': return true;
        default: return false;
    }
}
ZSW_SAM_HD bool ciglet_ok(uint32_t inc, uint8_t op) { return inc != 0 && op_ok(op); }

ZSW_SAM_HD uint32_t dec_digits32(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
ZSW_SAM_HD uint32_t dec_digits(uint64_t v) {
    if (v <= 0xffffffffull) return dec_digits32((uint32_t)v);
    uint32_t n = 10;
    for (uint64_t p = 10000000000ull; n < 20 && v >= p; p *= 10) ++n;  // 10^19 < 2^64: the last product that is taken fits
    return n;
}
// the characters ciglet (inc, op) takes: its decimal inc and the op byte
ZSW_SAM_HD uint32_t ciglet_chars(uint32_t inc) { return dec_digits32(inc) + 1u; }

// one ciglet, by the lane it belongs to
template <class Io>
ZSW_SAM_HD void put_ciglet(Io& io, uint64_t pos, uint32_t inc, uint8_t op) {
    const uint32_t nd = dec_digits32(inc);
    uint32_t v = inc;
    for (uint32_t k = nd; k-- > 0;) {
        io.put_lane(pos + k, (uint8_t)('0' + v % 10u));
        v /= 10u;
    }
    io.put_lane(pos + nd, op);
}

// the decimal writer of the uniform fields: v in nd = dec_digits(v) characters at pos, up to eight of them per put8
template <class Io>
ZSW_SAM_HD void put_dec(Io& io, uint64_t pos, uint64_t v, uint32_t nd) {
    while (nd) {
        const uint32_t c = nd > 8u ? 8u : nd;  // the last c digits, the least significant one into the highest byte
        uint64_t w = 0;
        if (v <= 0xffffffffull) {
            uint32_t v32 = (uint32_t)v;
            for (uint32_t t = 0; t < c; ++t) {
                w = (w << 8) | (uint64_t)('0' + v32 % 10u);
                v32 /= 10u;
            }
            v = v32;
        } else {
            for (uint32_t t = 0; t < c; ++t) {
                w = (w << 8) | (uint64_t)('0' + (uint32_t)(v % 10u));
                v /= 10u;
            }
        }
        nd -= c;
        io.put8(pos + nd, w, c);
    }
}

// what the walk needs to know of one read
struct Line {
    bool mapped;            // status SOME and a well-formed record: the long shape
    bool name_star;         // no qnames array: QNAME is "*"
    uint64_t name_len;
    bool seq_star;          // ZSW_SAM_OMIT_SEQ or a read of length 0
    bool qual_star;         // no quals array or a read of length 0
    bool reversed;          // strand != 0: FLAG 16, QUAL back to front
    uint64_t read_len;
    uint32_t rname_len, mapq;
    uint64_t pos;           // ref_start + 1
    uint32_t n_ciglets;
    uint64_t cigar_chars;   // of all ciglets together (the length walk; the write walk gets them from its sweeps)
    uint32_t score;
    bool has_nm;
    uint64_t nm;            // mismatches + ins_bases + del_bases
};

template <bool WRITE, class Io, int N>
ZSW_SAM_HD uint64_t text(Io& io, uint64_t p, const char (&s)[N]) {  // the N - 1 bytes of a literal
#pragma unroll
    for (int k = 0; k < N - 1; k += 8) {
        const int c = N - 1 - k < 8 ? N - 1 - k : 8;
        uint64_t w = 0;
#pragma unroll
        for (int j = 0; j < c; ++j) w |= (uint64_t)(uint8_t)s[k + j] << (8 * j);
        if (WRITE) io.put8(p + (uint64_t)k, w, (uint32_t)c);
    }
    return p + (uint64_t)(N - 1);
}
template <bool WRITE, class Io>
ZSW_SAM_HD uint64_t dec(Io& io, uint64_t p, uint64_t v) {
    const uint32_t nd = dec_digits(v);
    if (WRITE) put_dec(io, p, v, nd);
    return p + nd;
}

// the CIGAR in sweeps of SAM_G ciglets -> its characters; *bad: a ciglet with inc == 0 or an op outside MIDNSHP=X
template <bool WRITE, class Io>
ZSW_SAM_HD uint64_t cigar(Io& io, uint64_t p, uint32_t n_ciglets, bool* bad) {
    uint64_t chars = 0;
    for (uint64_t k0 = 0; k0 < n_ciglets; k0 += SAM_G) {
        const int nv = n_ciglets - k0 < (uint64_t)SAM_G ? (int)(n_ciglets - k0) : SAM_G;
        chars += io.template cigar_sweep<WRITE>(p + chars, k0, nv, bad);
    }
    return chars;
}

// The walk. Mapped:   QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ QUAL AS:i:score [NM:i:nm]   (FLAG 0 / 16; CIGAR "*" without ciglets)
//           unmapped: QNAME 4    *     0   0    *     * 0 0 SEQ QUAL
// tab-separated, closed by a newline. -> the length of the line.
template <bool WRITE, class Io>
ZSW_SAM_HD uint64_t line(Io& io, const Line& L) {
    uint64_t p = 0;
    if (L.name_star) {
        p = text<WRITE>(io, p, "*");
    } else {
        if (WRITE) io.name(p, L.name_len);
        p += L.name_len;
    }
    if (L.mapped) {
        p = L.reversed ? text<WRITE>(io, p, "\t16\t") : text<WRITE>(io, p, "\t0\t");
        if (WRITE) io.rname(p, L.rname_len);
        p += L.rname_len;
        p = text<WRITE>(io, p, "\t");
        p = dec<WRITE>(io, p, L.pos);
        p = text<WRITE>(io, p, "\t");
        p = dec<WRITE>(io, p, L.mapq);
        p = text<WRITE>(io, p, "\t");
        if (L.n_ciglets == 0) {
            p = text<WRITE>(io, p, "*");
        } else if (WRITE) {
            bool bad = false;
            p += cigar<true>(io, p, L.n_ciglets, &bad);
        } else {
            p += L.cigar_chars;
        }
        p = text<WRITE>(io, p, "\t*\t0\t0\t");
    } else {
        p = text<WRITE>(io, p, "\t4\t*\t0\t0\t*\t*\t0\t0\t");
    }
    if (L.seq_star) {
        p = text<WRITE>(io, p, "*");
    } else {
        if (WRITE) io.seq(p, L.read_len);
        p += L.read_len;
    }
    p = text<WRITE>(io, p, "\t");
    if (L.qual_star) {
        p = text<WRITE>(io, p, "*");
    } else {
        if (WRITE) io.qual(p, L.read_len, L.reversed);
        p += L.read_len;
    }
    if (L.mapped) {
        p = text<WRITE>(io, p, "\tAS:i:");
        p = dec<WRITE>(io, p, L.score);
        if (L.has_nm) {
            p = text<WRITE>(io, p, "\tNM:i:");
            p = dec<WRITE>(io, p, L.nm);
        }
    }
    return text<WRITE>(io, p, "\n");
}

template <class Io> ZSW_SAM_HD uint64_t line_length(Io& io, const Line& L) { return line<false>(io, L); }
template <class Io> ZSW_SAM_HD uint64_t write_line(Io& io, const Line& L) { return line<true>(io, L); }

// The fields of read i that do not depend on where the arrays live. A malformed record (ciglets outside [0, total), an inc of 0,
// an op outside MIDNSHP=X) is an unmapped line; *bad says so. The ciglets are only looked at when their range is good.
// verdict < 0: the ciglets are swept for their characters and their validity (the length launch); 0 / 1: what that sweep found
// for this read, mapped or not (the write launch, which then meets the ciglets once, as it writes them).
template <class Io>
ZSW_SAM_HD Line describe(Io& io, uint8_t status, const Rec& rec, uint64_t total_ciglets, bool have_names, uint64_t name_len, uint64_t read_len, bool have_quals,
                         bool omit_seq, bool reversed, uint32_t rname_len, uint32_t mapq, int verdict, bool* bad) {
    Line L{};
    L.name_star = !have_names;
    L.name_len = name_len;
    L.read_len = read_len;
    L.seq_star = omit_seq || read_len == 0;
    L.qual_star = !have_quals || read_len == 0;
    L.reversed = reversed;
    L.rname_len = rname_len;
    L.mapq = mapq;
    *bad = false;
    if (status == STATUS_SOME) {
        if (!ciglets_in_range(rec, total_ciglets)) {
            *bad = true;
        } else if (verdict < 0) {
            L.n_ciglets = rec.n_ciglets;
            L.cigar_chars = cigar<false>(io, 0, rec.n_ciglets, bad);
        } else {
            L.n_ciglets = rec.n_ciglets;
            *bad = verdict == 0;
        }
        L.mapped = !*bad;
    }
    if (!L.mapped) {
        L.n_ciglets = 0;
        L.cigar_chars = 0;
    }
    L.pos = (uint64_t)rec.ref_start + 1u;
    L.score = rec.score;
    return L;
}

}  // namespace sam
}  // namespace zsw
