// samtext_parse.cpp — host model of zsw_sam_parse_batch: zoe_amd/csrc/zsw_samtext.hpp (and zsw_text.hpp beneath it) compiled for the
// host, the same text the kernels compile, behind an Io that loops over the FQ_G lanes. The passes of zsw_samtext.hip in their order
// — the newline index, the line pass, the lowest failing index, the sums, the gather with the second CIGAR walk, the report — each
// array in a heap block of its exact size, so that a host sanitizer sees every load and store that leaves one.
//
//   samtext_parse FILE   one case per line:  <flags> <head 0..15> <ref_len> <rname as hex, - for none> <text as hex, - for empty>
//   output per case:     the thirteen report words, bases, qualities and names as hex (- for empty), offsets, name offsets, then per
//                        record status:score:ref_start:ref_end:query_start:query_end:ref_len:query_len:n_ciglets:ciglet_offset,
//                        the ciglets as inc:op, the strands, and per record pos:line:flag:mapq:code:bits (comma-separated, - for none)
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../zoe_amd/csrc/zsw_samtext.hpp"

using namespace zsw::samtext;

namespace {

template <class T>
struct Block {  // exactly n elements (one for n == 0, never touched)
    T* p;
    uint64_t n;
    explicit Block(uint64_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {}
    ~Block() { free(p); }
    Block(const Block&) = delete;
    T& at(uint64_t i) {
        if (i >= n) {
            fprintf(stderr, "model: index %llu outside a block of %llu\n", (unsigned long long)i, (unsigned long long)n);
            abort();
        }
        return p[i];
    }
};

struct LoopIo {
    Block<uint8_t>& text;
    uint64_t head;
    Block<uint64_t>* pos;
    Block<uint8_t>* rname;
    CigLane lanes[FQ_G];

    uint8_t byte(uint64_t p) const { return text.at(p); }
    void load16(uint64_t p, uint32_t w[4]) const {
        assert((p + head) % 16 == 0 && p + 16 <= text.n);
        for (int i = 0; i < 4; ++i) {
            w[i] = 0;
            for (int b = 0; b < 4; ++b) w[i] |= (uint32_t)text.at(p + 4 * i + b) << (8 * b);
        }
    }
    void stage(uint64_t lo, uint64_t hi) const { assert(lo <= hi && hi <= text.n); }
    uint64_t newline(uint64_t rank) const { return pos->at(rank); }
    void put_position(uint64_t rank, uint64_t p) const { pos->at(rank) = p; }
    bool sweep_utf8(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (int lane = 0; lane < FQ_G; ++lane)
            for (uint64_t j = (uint64_t)lane; j < n; j += FQ_G) bad |= utf8_bad_at(*this, lo, n, j);
        return bad;
    }
    bool sweep_quality(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (int lane = 0; lane < FQ_G; ++lane)
            for (uint64_t j = (uint64_t)lane; j < n; j += FQ_G) bad |= !quality_ok(byte(lo + j));
        return bad;
    }
    uint64_t mask_byte(uint64_t lo, uint64_t n, uint8_t c) const {
        assert(n <= (uint64_t)FQ_G);
        uint64_t m = 0;
        for (uint64_t lane = 0; lane < n; ++lane)
            if (byte(lo + lane) == c) m |= 1ull << lane;
        return m;
    }
    uint64_t sweep_byte(uint64_t lo, uint64_t n, uint8_t c) const {
        for (uint64_t j0 = 0; j0 < n; j0 += FQ_G)
            for (int lane = 0; lane < FQ_G; ++lane)
                if (j0 + lane < n && byte(lo + j0 + lane) == c) return j0 + lane;
        return n;
    }
    bool sweep_differs(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (int lane = 0; lane < FQ_G; ++lane)
            for (uint64_t j = (uint64_t)lane; j < n; j += FQ_G) bad |= byte(lo + j) != rname->at(j);
        return bad;
    }
    uint64_t cig_sweep(uint64_t c_lo, uint64_t lo, uint64_t n) {
        assert(n <= (uint64_t)FQ_G);
        uint64_t m = 0;
        for (uint64_t lane = 0; lane < n; ++lane)
            if (!is_digit(byte(lo + lane))) {
                lanes[lane] = cig_lane(*this, c_lo, lo + lane);
                m |= 1ull << lane;
            }
        return m;
    }
    CigLane cig_pick(uint32_t j) const { return lanes[j]; }
};

struct BlockSink {
    Block<uint32_t>& inc;
    Block<uint8_t>& op;
    uint64_t at, n;
    void put(uint64_t k, uint64_t i, uint32_t o) const {
        assert(k < n);
        inc.at(at + k) = (uint32_t)i;
        op.at(at + k) = (uint8_t)o;
    }
};

std::string hex(const uint8_t* p, uint64_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (uint64_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s.empty() ? "-" : s;
}

void unhex(const std::string& hx, Block<uint8_t>& out) {
    for (uint64_t i = 0; i < out.n; ++i) out.at(i) = (uint8_t)strtoul(hx.substr(2 * i, 2).c_str(), nullptr, 16);
}

void run_case(int flags, uint64_t head, uint32_t ref_len, const std::string& rname_hx, const std::string& hx) {
    const uint64_t n = hx == "-" ? 0 : hx.size() / 2;
    Block<uint8_t> text(n);
    unhex(hx, text);
    const uint32_t rname_len = rname_hx == "-" ? 0 : (uint32_t)(rname_hx.size() / 2);
    Block<uint8_t> rname(rname_len);
    unhex(rname_hx, rname);
    // the newline index
    const uint64_t n_tiles = tiles_of(head, n);
    Block<uint64_t> counts(n_tiles + 1), base(n_tiles + 1);
    LoopIo io{text, head, nullptr, &rname, {}};
    for (uint64_t t = 0; t < n_tiles; ++t) {
        uint64_t c = 0;
        for (uint64_t g = t * (FQ_TILE / 16); g < (t + 1) * (FQ_TILE / 16); ++g) {
            uint32_t w[4];
            granule_words(io, head, n, g, w);
            c += words_newlines(w);
        }
        counts.at(t) = c;
    }
    counts.at(n_tiles) = 0;
    uint64_t sum = 0;
    for (uint64_t t = 0; t <= n_tiles; ++t) {
        base.at(t) = sum;
        sum += counts.at(t);
    }
    const uint64_t n_nl = base.at(n_tiles);
    Block<uint64_t> pos(n_nl);
    io.pos = &pos;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        uint64_t rank = base.at(t);
        for (uint64_t g = t * (FQ_TILE / 16); g < (t + 1) * (FQ_TILE / 16); ++g) {
            uint32_t w[4];
            granule_words(io, head, n, g, w);
            rank += put_newlines(io, w, head, g, rank, n_nl);
        }
        assert(rank == base.at(t + 1));
    }
    // lines
    const Text t{n, n_nl, flags};
    const uint64_t lines = n_lines(t, n ? text.at(n - 1) == '\n' : true);
    Block<Line> line(lines);
    uint64_t first_bad = ~0ull;
    for (uint64_t L = lines; L-- > 0;) {  // any order: the lowest failing index is a minimum
        line.at(L) = parse_line(io, t, L, rname_len);
        if (line.at(L).code && L < first_bad) first_bad = L;
    }
    const uint64_t d = first_bad < lines ? first_bad : lines;
    // sums over the delivered lines
    Block<uint64_t> rec_of(d + 1), seq_off(d + 1), name_off(d + 1), cig_off(d + 1);
    uint64_t records = 0, bases = 0, names = 0, ciglets = 0, mapped = 0, coded = 0, lo = ~0ull, hi = 0;
    for (uint64_t L = 0; L < d; ++L) {
        const Line& R = line.at(L);
        rec_of.at(L) = records;
        seq_off.at(L) = bases;
        name_off.at(L) = names;
        cig_off.at(L) = ciglets;
        if (R.kind != KIND_DATA) continue;
        ++records;
        bases += R.seq_len;
        names += R.name_len;
        ciglets += R.n_ciglets;
        mapped += R.status == ST_SOME;
        coded += R.rec_code != 0;
        lo = R.seq_len < lo ? R.seq_len : lo;
        hi = R.seq_len > hi ? R.seq_len : hi;
    }
    rec_of.at(d) = records;
    seq_off.at(d) = bases;
    name_off.at(d) = names;
    cig_off.at(d) = ciglets;
    // the stated bounds always suffice
    assert(bases <= n && names <= n && ciglets <= n / 2 && records <= n / 14 + 1);
    // gather
    Block<uint8_t> out_bases(bases), out_quals(bases), out_names(names), out_status(records), out_op(ciglets), out_strand(records);
    Block<uint64_t> out_off(records + 1), out_noff(records + 1);
    Block<uint32_t> out_inc(ciglets);
    std::ostringstream recs, parsed, strands;
    for (uint64_t L = 0; L < d; ++L) {
        const Line& R = line.at(L);
        if (R.kind != KIND_DATA) continue;
        const uint64_t r = rec_of.at(L), s0 = seq_off.at(L), n0 = name_off.at(L), c0 = cig_off.at(L);
        const bool back = (flags & SF_QUAL_FORWARD) && (R.flag & 16u);
        for (uint64_t j = 0; j < R.seq_len; ++j) {
            out_bases.at(s0 + j) = text.at(R.seq_lo + j);
            out_quals.at(s0 + j) = R.qual_fill ? (uint8_t)'!' : text.at(R.qual_lo + (back ? R.seq_len - 1 - j : j));
        }
        for (uint64_t j = 0; j < R.name_len; ++j) out_names.at(n0 + j) = text.at(R.name_lo + j);
        out_off.at(r) = s0;
        out_noff.at(r) = n0;
        out_status.at(r) = (uint8_t)R.status;
        out_strand.at(r) = (R.flag & 16u) ? 1 : 0;
        const bool some = R.status == ST_SOME;
        recs << (r ? "," : "") << R.status << ':' << R.score << ':' << R.ref_start << ':' << R.ref_end << ':' << R.query_start << ':' << R.query_end << ':'
             << (some ? ref_len : 0u) << ':' << (some ? R.seq_len : 0) << ':' << R.n_ciglets << ':' << (some ? c0 : 0);
        parsed << (r ? "," : "") << R.pos << ':' << L << ':' << R.flag << ':' << R.mapq << ':' << R.rec_code << ':' << R.bits;
        strands << (r ? "," : "") << (int)out_strand.at(r);
        if (R.n_ciglets) {
            BlockSink sink{out_inc, out_op, c0, R.n_ciglets};
            const Cigar C = walk_cigar(io, R.cig_lo, R.cig_lo + R.cig_len, sink);
            assert(C.n_merged == R.n_ciglets && !C.err);
        }
    }
    out_off.at(records) = bases;
    out_noff.at(records) = names;
    uint64_t info[SI_WORDS] = {};
    info[SI_RECORDS] = records;
    info[SI_HEADERS] = d - records;
    info[SI_BASES] = bases;
    info[SI_NAME_BYTES] = names;
    info[SI_CIGLETS] = ciglets;
    info[SI_CONSUMED] = line_start(io, t, d);
    if (d < lines) {
        info[SI_ERROR] = line.at(d).code;
        info[SI_ERROR_LINE] = d;
        info[SI_ERROR_OFFSET] = line_start(io, t, d);
    }
    info[SI_MAPPED] = mapped;
    info[SI_CODED] = coded;
    info[SI_MIN_LEN] = records ? lo : 0;
    info[SI_MAX_LEN] = hi;
    for (int k = 0; k < SI_WORDS; ++k) std::cout << info[k] << ' ';
    std::cout << hex(out_bases.p, bases) << ' ' << hex(out_quals.p, bases) << ' ' << hex(out_names.p, names) << ' ';
    for (uint64_t r = 0; r <= records; ++r) std::cout << (r ? "," : "") << out_off.at(r);
    std::cout << ' ';
    for (uint64_t r = 0; r <= records; ++r) std::cout << (r ? "," : "") << out_noff.at(r);
    std::cout << ' ' << (records ? recs.str() : "-") << ' ';
    for (uint64_t k = 0; k < ciglets; ++k) std::cout << (k ? "," : "") << out_inc.at(k) << ':' << (int)out_op.at(k);
    if (!ciglets) std::cout << '-';
    std::cout << ' ' << (records ? strands.str() : "-") << ' ' << (records ? parsed.str() : "-") << '\n';
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        int flags;
        uint64_t head;
        uint32_t ref_len;
        std::string rname, hx;
        if (!(ss >> flags >> head >> ref_len >> rname >> hx) || head > 15) return 2;
        run_case(flags, head, ref_len, rname, hx);
    }
    return 0;
}
