// sam_line.cpp — host model of zsw_sam_batch: zoe_amd/csrc/zsw_sam.hpp compiled for the host, the same text the kernel
// (zoe_amd/csrc/zsw_sam.hip) compiles. The walk over a line's fields, dec_digits and the decimal writers, the characters of a
// ciglet, the validity rules and describe() run here exactly as on the device; the Io behind them loops over the SAM_G lanes where
// the kernel has a wavefront. The model requires what the two launches rely on:
//   line_length() == the length write_line() returns == the number of bytes put,
//   every byte of the line is put exactly once, none outside it.
// What it does not cover: the kernel's own Io (WaveIo), the LDS assembly and its flush, the scan, the launches and the entry
// point's argument checks; tests/test_gpu_sam.py compares those with tests/sam_ref.py on the device.
//
// Every array sits in a heap block of exactly its size, so that -fsanitize=address,undefined sees any index derived from a
// malformed record (tests/test_sam_model.py runs the malformed records through such a build).
//
// usage: sam_line <cases.txt>   (format: read_cases below; one result line per case on stdout)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../zoe_amd/csrc/zsw_sam.hpp"

using namespace zsw::sam;

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "%s\n", what);
    exit(3);
}

struct HostIo {
    uint8_t* out = nullptr;  // the line: len bytes
    uint32_t* puts = nullptr;  // how often each byte was put
    uint64_t len = 0;
    const uint8_t *p_name = nullptr, *p_rname = nullptr, *p_seq = nullptr, *p_qual = nullptr;
    const uint32_t* inc = nullptr;  // the record's ciglets
    const uint8_t* op = nullptr;

    void put(uint64_t pos, uint8_t b) {
        if (pos >= len) die("a byte put outside the line");
        out[pos] = b;
        ++puts[pos];
    }
    void put8(uint64_t pos, uint64_t w, uint32_t n) {
        if (n > 8) die("put8 of more than eight bytes");
        for (uint32_t lane = 0; lane < n; ++lane) put(pos + lane, (uint8_t)(w >> (8 * lane)));
    }
    void put_lane(uint64_t pos, uint8_t b) { put(pos, b); }
    void copy(uint64_t pos, const uint8_t* src, uint64_t n, bool reversed) {
        for (uint64_t j = 0; j < n; ++j) put(pos + j, src[reversed ? n - 1 - j : j]);
    }
    void name(uint64_t pos, uint64_t n) { copy(pos, p_name, n, false); }
    void rname(uint64_t pos, uint64_t n) { copy(pos, p_rname, n, false); }
    void seq(uint64_t pos, uint64_t n) { copy(pos, p_seq, n, false); }
    void qual(uint64_t pos, uint64_t n, bool reversed) { copy(pos, p_qual, n, reversed); }
    template <bool WRITE>
    uint32_t cigar_sweep(uint64_t pos, uint64_t k0, int nv, bool* bad) {
        if (nv < 1 || nv > SAM_G) die("a sweep of no or too many ciglets");
        uint32_t chars = 0;
        for (int lane = 0; lane < nv; ++lane) {
            const uint32_t i = inc[k0 + lane];
            const uint8_t o = op[k0 + lane];
            if (!ciglet_ok(i, o)) {
                *bad = true;
                continue;
            }
            if (WRITE) put_ciglet(*this, pos + chars, i, o);
            chars += ciglet_chars(i);
        }
        return chars;
    }
};

std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> v;
    if (!strcmp(s, "-")) return v;
    auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
    for (; s[0] && s[1]; s += 2) v.push_back((uint8_t)(nib(s[0]) * 16 + nib(s[1])));
    return v;
}

template <typename T>
T* exact(const std::vector<T>& v) {  // a heap block of exactly the array's size
    T* p = (T*)malloc(v.size() * sizeof(T));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

void run_dec(unsigned long long v) {
    const uint32_t nd = dec_digits(v);
    std::vector<uint8_t> line(nd, 0);
    std::vector<uint32_t> puts(nd, 0);
    HostIo io;
    io.out = line.data();
    io.puts = puts.data();
    io.len = nd;
    put_dec(io, 0, v, nd);
    for (uint32_t k = 0; k < nd; ++k)
        if (puts[k] != 1) die("a digit put twice or not at all");
    printf("%u %.*s\n", nd, (int)nd, (const char*)line.data());
}

struct Case {
    int flags, status, have_names, have_quals, strand, have_stats;
    std::vector<uint8_t> name, qual, read, rname;
    uint32_t mismatches, ins_bases, del_bases, mapq;
    Rec rec;
    std::vector<uint32_t> inc;
    std::vector<uint8_t> op;
};

void run_case(const Case& c) {
    uint8_t *nm = exact(c.name), *ql = exact(c.qual), *rd = exact(c.read), *rn = exact(c.rname), *op = exact(c.op);
    uint32_t* inc = exact(c.inc);
    HostIo io;
    io.p_name = c.have_names ? nm : nullptr;
    io.p_rname = rn;
    io.p_seq = rd;
    io.p_qual = c.have_quals ? ql : nullptr;
    const bool in_range = ciglets_in_range(c.rec, c.inc.size());
    io.inc = in_range ? inc + c.rec.ciglet_offset : nullptr;
    io.op = in_range ? op + c.rec.ciglet_offset : nullptr;
    auto with_nm = [&](Line L) {
        if (c.have_stats && L.mapped) {
            L.has_nm = true;
            L.nm = (uint64_t)c.mismatches + (uint64_t)c.ins_bases + (uint64_t)c.del_bases;
        }
        return L;
    };
    // the length launch
    bool bad = false;
    const Line L = with_nm(describe(io, (uint8_t)c.status, c.rec, c.inc.size(), c.have_names != 0, c.name.size(), c.read.size(), c.have_quals != 0,
                                    (c.flags & F_OMIT_SEQ) != 0, c.strand > 0, (uint32_t)c.rname.size(), c.mapq, -1, &bad));
    const uint64_t len = line_length(io, L);
    // the write launch: the verdict of the length launch, the bytes of the scan
    bool bad2 = false;
    const Line L2 = with_nm(describe(io, (uint8_t)c.status, c.rec, c.inc.size(), c.have_names != 0, c.name.size(), c.read.size(), c.have_quals != 0,
                                     (c.flags & F_OMIT_SEQ) != 0, c.strand > 0, (uint32_t)c.rname.size(), c.mapq, L.mapped ? 1 : 0, &bad2));
    if (L2.mapped != L.mapped) die("the write launch takes another shape than the length launch");
    std::vector<uint32_t> puts(len, 0);
    io.out = (uint8_t*)malloc(len);
    io.puts = puts.data();
    io.len = len;
    const uint64_t written = write_line(io, L2);
    if (written != len) die("write_line() and line_length() disagree");
    for (uint64_t k = 0; k < len; ++k)
        if (puts[k] != 1) die("a byte of the line put twice or not at all");
    printf("%d %llu ", bad ? 1 : 0, (unsigned long long)len);
    for (uint64_t k = 0; k < len; ++k) printf("%02x", io.out[k]);
    printf("\n");
    free(io.out);
    free(nm);
    free(ql);
    free(rd);
    free(rn);
    free(op);
    free(inc);
}

// any number of
//   dec <v>                                            dec_digits(v) and the decimal writer's text
//   case flags status have_names <name hex | -> have_quals <qual hex | -> <read hex | -> strand have_stats mismatches ins_bases del_bases
//        <rname hex> mapq score ref_start n_ciglets ciglet_offset total, followed by `total` pairs "inc op" (op as a number): the
//        whole ciglet arrays of the call. strand: -1 = no strand array
int read_cases(FILE* f) {
    char word[64];
    std::string buf;
    while (fscanf(f, "%63s", word) == 1) {
        auto token = [&]() {
            buf.clear();
            int ch;
            while ((ch = fgetc(f)) != EOF && (ch == ' ' || ch == '\n')) {}
            for (; ch != EOF && ch != ' ' && ch != '\n'; ch = fgetc(f)) buf.push_back((char)ch);
            return buf.c_str();
        };
        if (!strcmp(word, "dec")) {
            unsigned long long v;
            if (fscanf(f, "%llu", &v) != 1) return 2;
            run_dec(v);
        } else if (!strcmp(word, "case")) {
            Case c{};
            if (fscanf(f, "%d %d %d", &c.flags, &c.status, &c.have_names) != 3) return 2;
            c.name = unhex(token());
            if (fscanf(f, "%d", &c.have_quals) != 1) return 2;
            c.qual = unhex(token());
            c.read = unhex(token());
            if (fscanf(f, "%d %d %u %u %u", &c.strand, &c.have_stats, &c.mismatches, &c.ins_bases, &c.del_bases) != 5) return 2;
            c.rname = unhex(token());
            unsigned long long off, total;
            if (fscanf(f, "%u %u %u %u %llu %llu", &c.mapq, &c.rec.score, &c.rec.ref_start, &c.rec.n_ciglets, &off, &total) != 6) return 2;
            c.rec.ciglet_offset = off;
            if (c.have_quals && c.qual.size() != c.read.size()) return 2;
            c.inc.resize(total);
            c.op.resize(total);
            for (unsigned long long k = 0; k < total; ++k) {
                unsigned o;
                if (fscanf(f, "%u %u", &c.inc[k], &o) != 2) return 2;
                c.op[k] = (uint8_t)o;
            }
            run_case(c);
        } else {
            return 2;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <cases.txt>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    const int rc = read_cases(f);
    fclose(f);
    if (rc) fprintf(stderr, "malformed case file\n");
    return rc;
}
