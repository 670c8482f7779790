// fasta_parse.cpp — host model of zsw_fasta_parse_batch: zoe_amd/csrc/zsw_fasta.hpp (and zsw_text.hpp beneath it) compiled for the host, the same text the
// kernels compile, behind an Io that loops over the FQ_G lanes. The passes of zsw_fasta.hip in their order — '>' per tile, their
// exclusive sum, positions by rank, the start of the file, the record pass, the lowest failing index, the name offsets, the kept bytes
// per tile, their exclusive sum, the write sweep, the gather, the report — each array in a heap block of its exact size, so that a
// host sanitizer sees every load and store that leaves one.
//
//   fasta_parse FILE     one case per line:  <flags> <head 0..15> <text as hex, - for empty>
//   output per case:     the nine report words, bases and names as hex (- for empty), offsets and name offsets (comma-separated);
//                        "invalid" for a CONTINUED text that does not start with '>'
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../zoe_amd/csrc/zsw_fasta.hpp"

using namespace zsw::fasta;

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
    Block<uint64_t>* body;
    Block<uint8_t>* bases;
    Block<uint64_t>* off;

    uint8_t byte(uint64_t p) const { return text.at(p); }
    void load16(uint64_t p, uint32_t w[4]) const {
        assert((p + head) % 16 == 0 && p + 16 <= text.n);
        for (int i = 0; i < 4; ++i) {
            w[i] = 0;
            for (int b = 0; b < 4; ++b) w[i] |= (uint32_t)text.at(p + 4 * i + b) << (8 * b);
        }
    }
    uint64_t newline(uint64_t rank) const { return pos->at(rank); }
    void put_position(uint64_t rank, uint64_t p) const { pos->at(rank) = p; }
    uint64_t sweep_class(uint64_t lo, uint64_t n, int cls) const {
        for (uint64_t j0 = 0; j0 < n; j0 += FQ_G)
            for (int lane = 0; lane < FQ_G; ++lane)
                if (j0 + lane < n && in_class(byte(lo + j0 + lane), cls)) return j0 + lane;
        return n;
    }
    uint64_t sweep_class_last(uint64_t lo, uint64_t n, int cls) const {
        for (uint64_t j0 = 0; j0 < n; j0 += FQ_G)
            for (int lane = 0; lane < FQ_G; ++lane)
                if (j0 + lane < n && in_class(byte(lo + n - 1 - (j0 + lane)), cls)) return n - 1 - (j0 + lane);
        return n;
    }
    uint64_t body_lo(uint64_t r) const { return body->at(r); }
    void put_base(uint64_t rank, uint8_t c) const { bases->at(rank) = c; }
    void put_offset(uint64_t r, uint64_t kept) const { off->at(r) = kept; }
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

void run_case(int flags, uint64_t head, const std::string& hx) {
    const uint64_t n = hx == "-" ? 0 : hx.size() / 2;
    Block<uint8_t> text(n);
    for (uint64_t i = 0; i < n; ++i) text.at(i) = (uint8_t)strtoul(hx.substr(2 * i, 2).c_str(), nullptr, 16);
    if ((flags & F_CONTINUED) && (!n || text.at(0) != '>')) {
        std::cout << "invalid\n";
        return;
    }
    const uint64_t per_tile = FQ_TILE / 16;
    // count the '>'
    const uint64_t n_tiles = tiles_of(head, n);
    Block<uint64_t> counts(n_tiles + 1), base(n_tiles + 1);
    LoopIo io{text, head, nullptr, nullptr, nullptr, nullptr};
    for (uint64_t t = 0; t < n_tiles; ++t) {
        uint64_t c = 0;
        for (uint64_t g = t * per_tile; g < (t + 1) * per_tile; ++g) {
            uint32_t w[4];
            granule_words(io, head, n, g, w);
            c += words_newlines<'>'>(w);
        }
        counts.at(t) = c;
    }
    counts.at(n_tiles) = 0;
    uint64_t sum = 0;
    for (uint64_t t = 0; t <= n_tiles; ++t) {
        base.at(t) = sum;
        sum += counts.at(t);
    }
    const uint64_t n_gt = base.at(n_tiles);
    uint64_t plain = 0;
    for (uint64_t i = 0; i < n; ++i) plain += text.at(i) == '>';
    assert(plain == n_gt);
    // positions
    Block<uint64_t> pos(n_gt);
    io.pos = &pos;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        uint64_t rank = base.at(t);
        for (uint64_t g = t * per_tile; g < (t + 1) * per_tile; ++g) {
            uint32_t w[4];
            granule_words(io, head, n, g, w);
            rank += put_newlines<'>'>(io, w, head, g, rank, n_gt);
        }
        assert(rank == base.at(t + 1));
    }
    for (uint64_t k = 0; k < n_gt; ++k) assert(text.at(pos.at(k)) == '>' && (!k || pos.at(k - 1) < pos.at(k)));
    // the start of the file, the records
    const Text t{n, n_gt, flags};
    const uint64_t n_rec = n_records(t, false);
    Start start{};
    if (!(flags & F_CONTINUED)) start = check_start(io, t);
    Block<uint8_t> code(n_rec);
    Block<uint64_t> name_len(n_rec), body(n_rec);
    io.body = &body;
    uint64_t first_bad = start.code ? 0 : ~0ull;
    for (uint64_t r = n_rec; r-- > 0;) {  // any order: the lowest failing index is a minimum
        const Record R = parse_record(io, t, r);
        code.at(r) = (uint8_t)R.code;
        name_len.at(r) = R.name_len;
        body.at(r) = R.body_lo;
        if (R.code && r < first_bad) first_bad = r;
    }
    const uint64_t delivered = first_bad < n_rec ? first_bad : n_rec;
    const uint64_t cut = gt_at(io, t, delivered);
    Block<uint64_t> name_off(delivered + 1);
    uint64_t names = 0;
    for (uint64_t r = 0; r < delivered; ++r) {
        name_off.at(r) = names;
        names += name_len.at(r);
    }
    name_off.at(delivered) = names;
    // the sequence pass: kept bytes per tile, their sum, the write sweep
    Block<uint64_t> kept(n_tiles + 1), kept_base(n_tiles + 1);
    for (uint64_t tl = 0; tl < n_tiles; ++tl) {
        uint64_t c = 0, gts = base.at(tl);
        for (uint64_t g = tl * per_tile; g < (tl + 1) * per_tile; ++g) {
            uint32_t w[4];
            granule_words(io, head, n, g, w);
            c += granule_bases<false>(io, w, head, n, g, gts, n_rec, cut, 0);
            gts += words_newlines<'>'>(w);
        }
        kept.at(tl) = c;
    }
    kept.at(n_tiles) = 0;
    sum = 0;
    for (uint64_t tl = 0; tl <= n_tiles; ++tl) {
        kept_base.at(tl) = sum;
        sum += kept.at(tl);
    }
    const uint64_t bases = kept_base.at(n_tiles);
    Block<uint8_t> out_bases(bases), out_names(names);
    Block<uint64_t> off(n_gt);
    io.bases = &out_bases;
    io.off = &off;
    for (uint64_t tl = n_tiles; tl-- > 0;) {  // any order
        uint64_t rank = kept_base.at(tl), gts = base.at(tl);
        for (uint64_t g = tl * per_tile; g < (tl + 1) * per_tile; ++g) {
            uint32_t w[4];
            granule_words(io, head, n, g, w);
            rank += granule_bases<true>(io, w, head, n, g, gts, n_rec, cut, rank);
            gts += words_newlines<'>'>(w);
        }
        assert(rank == kept_base.at(tl + 1));
    }
    // the stated bounds always suffice
    assert(bases <= n && names <= n && delivered <= n / 4 + 1);
    // gather
    Block<uint64_t> seq_off(delivered + 1);
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t r = 0; r < delivered; ++r) {
        const uint64_t s0 = off.at(r), s1 = r + 1 < delivered ? off.at(r + 1) : bases;
        assert(s1 > s0);
        seq_off.at(r) = s0;
        lo = s1 - s0 < lo ? s1 - s0 : lo;
        hi = s1 - s0 > hi ? s1 - s0 : hi;
        const uint64_t n_lo = name_start(io, t, r);
        for (uint64_t j = 0; j < name_len.at(r); ++j) out_names.at(name_off.at(r) + j) = text.at(n_lo + j);
    }
    seq_off.at(delivered) = bases;
    uint64_t info[INFO_WORDS] = {};
    info[INFO_RECORDS] = delivered;
    info[INFO_BASES] = bases;
    info[INFO_NAME_BYTES] = names;
    info[INFO_CONSUMED] = start.code ? 0 : n_gt ? cut : start.consumed;
    if (start.code) {
        info[INFO_ERROR] = start.code;
        info[INFO_ERROR_OFFSET] = start.offset;
    } else if (delivered < n_rec) {
        info[INFO_ERROR] = code.at(delivered);
        info[INFO_ERROR_RECORD] = delivered;
        info[INFO_ERROR_OFFSET] = cut;
    }
    info[INFO_MIN_LEN] = delivered ? lo : 0;
    info[INFO_MAX_LEN] = hi;
    for (int k = 0; k < INFO_WORDS; ++k) std::cout << info[k] << ' ';
    std::cout << hex(out_bases.p, bases) << ' ' << hex(out_names.p, names) << ' ';
    for (uint64_t r = 0; r <= delivered; ++r) std::cout << (r ? "," : "") << seq_off.at(r);
    std::cout << ' ';
    for (uint64_t r = 0; r <= delivered; ++r) std::cout << (r ? "," : "") << name_off.at(r);
    std::cout << '\n';
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
        std::string hx;
        if (!(ss >> flags >> head >> hx) || head > 15) return 2;
        run_case(flags, head, hx);
    }
    return 0;
}
