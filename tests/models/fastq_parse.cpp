// fastq_parse.cpp — host model of zsw_fastq_parse_batch: zoe_amd/csrc/zsw_fastq.hpp (and zsw_text.hpp beneath it) compiled for the host, the same text the
// kernels compile, behind an Io that loops over the FQ_G lanes. The passes of zsw_fastq.hip in their order — newlines per tile, their
// exclusive sum, positions by rank, the record pass, the lowest failing index, the offsets, the gather, the report — each array in a
// heap block of its exact size, so that a host sanitizer sees every load and store that leaves one.
//
//   fastq_parse FILE     one case per line:  <flags> <head 0..15> <text as hex, - for empty>
//   output per case:     the nine report words, bases, qualities and names as hex (- for empty), offsets and name offsets (comma-separated)
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../zoe_amd/csrc/zsw_fastq.hpp"

using namespace zsw::fastq;

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
    uint64_t sweep_blank(uint64_t lo, uint64_t n) const {
        for (uint64_t j0 = 0; j0 < n; j0 += FQ_G)
            for (int lane = 0; lane < FQ_G; ++lane)
                if (j0 + lane < n && is_blank(byte(lo + j0 + lane))) return j0 + lane;
        return n;
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

void run_case(int flags, uint64_t head, const std::string& hx) {
    const uint64_t n = hx == "-" ? 0 : hx.size() / 2;
    Block<uint8_t> text(n);
    for (uint64_t i = 0; i < n; ++i) text.at(i) = (uint8_t)strtoul(hx.substr(2 * i, 2).c_str(), nullptr, 16);
    // count
    const uint64_t n_tiles = tiles_of(head, n);
    Block<uint64_t> counts(n_tiles + 1), base(n_tiles + 1);
    LoopIo io{text, head, nullptr};
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
    uint64_t plain = 0;
    for (uint64_t i = 0; i < n; ++i) plain += text.at(i) == '\n';
    assert(plain == n_nl);
    // positions
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
    for (uint64_t k = 0; k < n_nl; ++k) assert(text.at(pos.at(k)) == '\n' && (!k || pos.at(k - 1) < pos.at(k)));
    // records
    const Text t{n, n_nl, flags};
    const uint64_t n_rec = n_records(t, n ? text.at(n - 1) == '\n' : true);
    Block<uint8_t> code(n_rec);
    Block<uint64_t> name_len(n_rec), seq_len(n_rec);
    uint64_t first_bad = ~0ull;
    for (uint64_t r = n_rec; r-- > 0;) {  // any order: the lowest failing index is a minimum
        const Record R = parse_record(io, t, r);
        code.at(r) = (uint8_t)R.code;
        name_len.at(r) = R.name_len;
        seq_len.at(r) = R.seq_len;
        if (R.code && r < first_bad) first_bad = r;
    }
    const uint64_t delivered = first_bad < n_rec ? first_bad : n_rec;
    Block<uint64_t> seq_off(delivered + 1), name_off(delivered + 1);
    uint64_t bases = 0, names = 0, lo = ~0ull, hi = 0;
    for (uint64_t r = 0; r < delivered; ++r) {
        seq_off.at(r) = bases;
        name_off.at(r) = names;
        bases += seq_len.at(r);
        names += name_len.at(r);
        lo = seq_len.at(r) < lo ? seq_len.at(r) : lo;
        hi = seq_len.at(r) > hi ? seq_len.at(r) : hi;
    }
    seq_off.at(delivered) = bases;
    name_off.at(delivered) = names;
    // the stated bounds always suffice
    assert(bases <= n / 2 && names <= n && delivered <= n / 8 + 1);
    // gather
    Block<uint8_t> out_bases(bases), out_quals(bases), out_names(names);
    for (uint64_t r = 0; r < delivered; ++r) {
        const Record R = locate_record(io, t, r);
        for (uint64_t j = 0; j < seq_len.at(r); ++j) {
            out_bases.at(seq_off.at(r) + j) = text.at(R.seq_lo + j);
            out_quals.at(seq_off.at(r) + j) = text.at(R.qual_lo + j);
        }
        for (uint64_t j = 0; j < name_len.at(r); ++j) out_names.at(name_off.at(r) + j) = text.at(R.name_lo + j);
    }
    uint64_t info[INFO_WORDS] = {};
    info[INFO_RECORDS] = delivered;
    info[INFO_BASES] = bases;
    info[INFO_NAME_BYTES] = names;
    info[INFO_CONSUMED] = line_start(io, t, 4 * delivered);
    if (delivered < n_rec) {
        info[INFO_ERROR] = code.at(delivered);
        info[INFO_ERROR_RECORD] = delivered;
        info[INFO_ERROR_OFFSET] = line_start(io, t, 4 * delivered);
    }
    info[INFO_MIN_LEN] = delivered ? lo : 0;
    info[INFO_MAX_LEN] = hi;
    for (int k = 0; k < INFO_WORDS; ++k) std::cout << info[k] << ' ';
    std::cout << hex(out_bases.p, bases) << ' ' << hex(out_quals.p, bases) << ' ' << hex(out_names.p, names) << ' ';
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
