// pileup_walk.cpp — host model of zsw_pileup_batch and zsw_consensus_from_counts: zoe_amd/csrc/zsw_pileup.hpp compiled for the
// host, the same text the kernels (zoe_amd/csrc/zsw_pileup.hip) compile. The bin table, record_ok() and validate() before count(),
// the role swap, the decomposition into difference arrays plus per-site misses, their scan under combine() and resolve_site(), and
// the vote run here exactly as on the device; the Io behind the walks loops over the PILEUP_G lanes where the kernel has a
// wavefront (ciglets fetched PILEUP_G at a time, one column per lane, the two ends of a range by two lanes). What this model does
// not cover: the kernel's own Io (WaveIo) with its atomics, the LDS accumulators and their flush, hipcub's scan, the launches and
// the entry points' argument checks and staging; tests/test_gpu_pileup.py compares those with tests/pileup_ref.py on the device.
//
// Every array sits in a heap block of exactly its size, so that -fsanitize=address,undefined sees any index the walks derive from
// a malformed record (tests/test_pileup_model.py runs the malformed records through such a build).
//
// usage: pileup_walk <cases.txt>   (format: read_cases below)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../zoe_amd/csrc/zsw_pileup.hpp"

using namespace zsw::pile;
namespace ann = zsw::ann;

namespace {

struct HostIo {
    const uint8_t *read, *seq_bins;
    uint32_t *acc, *counts, *ins;
    const uint32_t* inc;  // the record's ciglets
    const uint8_t* op;
    uint32_t n_ciglets;
    uint32_t c_inc[PILEUP_G], c_op[PILEUP_G];

    void ciglet(uint32_t k, uint32_t* i, uint8_t* o) {
        const uint32_t slot = k & (PILEUP_G - 1);
        if (slot == 0)
            for (int lane = 0; lane < PILEUP_G; ++lane) {
                c_inc[lane] = 0;
                c_op[lane] = 0;
                if ((uint64_t)k + lane < n_ciglets) {
                    c_inc[lane] = inc[k + lane];
                    c_op[lane] = op[k + lane];
                }
            }
        *i = c_inc[slot];
        *o = (uint8_t)c_op[slot];
    }
    void range(int which, uint64_t site, uint32_t n) {
        for (int lane = 0; lane < 2; ++lane) acc[(site + (lane ? n : 0u)) * D_FIELDS + which] += lane ? 0xffffffffu : 1u;
    }
    void columns(uint64_t site, uint64_t rd, int nv) {
        for (int lane = 0; lane < PILEUP_G; ++lane) {
            if (lane >= nv) continue;
            const int b = bin_of(read[rd + lane]), e = seq_bins[site + lane];
            if (b != e) {
                acc[(site + lane) * D_FIELDS + D_MISS] += 1u;
                counts[(site + lane) * N_BINS + b] += 1u;
            }
        }
    }
    void insertion(uint64_t p, uint32_t n) {
        for (int lane = 0; lane < 2; ++lane) ins[p * 2 + lane] += lane ? n : 1u;
    }
};

// exactly n elements on the heap (n == 0: a block of one byte that nothing may read is still a valid pointer)
template <typename T>
T* exact(const std::vector<T>& v) {
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    if (!strcmp(s, "-")) return out;
    for (size_t k = 0; s[k] && s[k + 1]; k += 2) {
        unsigned v = 0;
        sscanf(s + k, "%2x", &v);
        out.push_back((uint8_t)v);
    }
    return out;
}

// The table of one call: the caller's tables and the workspace, each a heap block of its exact size
struct Table {
    uint32_t len = 0;
    uint8_t* seq_bins = nullptr;
    uint32_t *acc = nullptr, *counts = nullptr, *ins = nullptr;
    unsigned long long n_bad = 0;

    void release() {
        free(seq_bins);
        free(acc);
        free(counts);
        free(ins);
        seq_bins = nullptr;
        acc = counts = ins = nullptr;
    }
    void start(const std::vector<uint8_t>& seq) {
        release();
        len = (uint32_t)seq.size();
        std::vector<uint8_t> bins(len);
        for (uint32_t k = 0; k < len; ++k) bins[k] = (uint8_t)bin_of(seq[k]);
        seq_bins = exact(bins);
        acc = exact(std::vector<uint32_t>((size_t)(len + 1) * D_FIELDS, 0u));
        counts = exact(std::vector<uint32_t>((size_t)len * N_BINS, 0u));
        ins = exact(std::vector<uint32_t>((size_t)(len + 1) * 2, 0u));
        n_bad = 0;
    }
    // one read as the kernel treats it
    void add(int flags, int status, const std::vector<uint8_t>& read, const Rec& rec, const std::vector<uint32_t>& inc_v, const std::vector<uint8_t>& op_v) {
        if (status != 0) return;
        uint8_t *rd = exact(read), *op = exact(op_v);
        uint32_t* inc = exact(inc_v);
        const bool swap = (flags & F_READ_IS_REF) != 0;
        const uint32_t rl = (uint32_t)read.size();
        bool ok = ann::record_ok(rec, inc_v.size(), swap ? rl : len, swap ? len : rl);
        HostIo io;
        if (ok) {
            io.read = rd;
            io.seq_bins = seq_bins;
            io.acc = acc;
            io.counts = counts;
            io.ins = ins;
            io.inc = inc + rec.ciglet_offset;
            io.op = op + rec.ciglet_offset;
            io.n_ciglets = rec.n_ciglets;
            ok = validate(io, rec);
        }
        if (!ok) ++n_bad;
        else count(io, rec, swap, true);
        free(rd);
        free(op);
        free(inc);
    }
    // the scan and the resolve launch, then the tables on stdout: n_bad / len lines of 8 bins / len + 1 lines "runs bases"
    void finish() {
        Diff* d = reinterpret_cast<Diff*>(acc);
        for (uint32_t k = 1; k <= len; ++k) d[k] = combine(d[k - 1], d[k]);
        for (uint32_t k = 0; k < len; ++k) resolve_site(counts + (size_t)k * N_BINS, d[k], seq_bins[k]);
        printf("%llu\n", n_bad);
        for (uint32_t k = 0; k < len; ++k) {
            for (int b = 0; b < N_BINS; ++b) printf(b ? " %u" : "%u", counts[(size_t)k * N_BINS + b]);
            printf("\n");
        }
        for (uint32_t k = 0; k <= len; ++k) printf("%u %u\n", ins[k * 2], ins[k * 2 + 1]);
    }
};

// Any number of
//   seq <hex | ->            starts a table over this sequence
//   case flags status <read hex | -> score ref_start ref_end query_start query_end ref_len query_len n_ciglets ciglet_offset total
//        followed by `total` pairs "inc op" (op as a number): the whole ciglet arrays of the call; the read is added to the table
//   table                    prints the table (see Table::finish) and ends it
//   bins <hex | ->           prints the bin of every byte, space-separated, on one line
//   plurality <hex | ->      the composition of the bytes as one site; prints plurality_acgtn as a number
//   consensus flags <fallback hex | -> n  then n lines of 8 bins   prints consensus_byte per site as numbers on one line
int read_cases(FILE* f) {
    Table t;
    bool open = false;
    char word[64];
    std::string buf;
    auto token = [&]() {
        buf.clear();
        int c;
        while ((c = fgetc(f)) != EOF && (c == ' ' || c == '\n')) {}
        for (; c != EOF && c != ' ' && c != '\n'; c = fgetc(f)) buf.push_back((char)c);
        return buf.c_str();
    };
    while (fscanf(f, "%63s", word) == 1) {
        if (!strcmp(word, "seq")) {
            t.start(unhex(token()));
            open = true;
        } else if (!strcmp(word, "case")) {
            int flags, status;
            if (!open || fscanf(f, "%d %d", &flags, &status) != 2) return 2;
            const std::vector<uint8_t> read = unhex(token());
            Rec rec;
            unsigned long long off, total;
            if (fscanf(f, "%u %u %u %u %u %u %u %u %llu %llu", &rec.score, &rec.ref_start, &rec.ref_end, &rec.query_start, &rec.query_end, &rec.ref_len,
                       &rec.query_len, &rec.n_ciglets, &off, &total) != 10)
                return 2;
            rec.ciglet_offset = off;
            std::vector<uint32_t> inc(total);
            std::vector<uint8_t> op(total);
            for (unsigned long long k = 0; k < total; ++k) {
                unsigned o;
                if (fscanf(f, "%u %u", &inc[k], &o) != 2) return 2;
                op[k] = (uint8_t)o;
            }
            t.add(flags, status, read, rec, inc, op);
        } else if (!strcmp(word, "table")) {
            if (!open) return 2;
            t.finish();
            t.release();
            open = false;
        } else if (!strcmp(word, "bins")) {
            const std::vector<uint8_t> s = unhex(token());
            for (size_t k = 0; k < s.size(); ++k) printf(k ? " %d" : "%d", bin_of(s[k]));
            printf("\n");
        } else if (!strcmp(word, "plurality")) {
            uint32_t bins[N_BINS] = {};
            for (uint8_t b : unhex(token())) ++bins[bin_of(b)];
            printf("%u\n", (unsigned)plurality_acgtn(bins));
        } else if (!strcmp(word, "consensus")) {
            int flags;
            if (fscanf(f, "%d", &flags) != 1) return 2;
            const std::vector<uint8_t> fb = unhex(token());
            unsigned n;
            if (fscanf(f, "%u", &n) != 1 || ((flags & K_KEEP_UNCOVERED) && fb.size() != n)) return 2;
            for (unsigned k = 0; k < n; ++k) {
                uint32_t bins[N_BINS];
                for (int b = 0; b < N_BINS; ++b)
                    if (fscanf(f, "%u", &bins[b]) != 1) return 2;
                printf(k ? " %u" : "%u", (unsigned)consensus_byte(bins, flags, (flags & K_KEEP_UNCOVERED) ? fb[k] : (uint8_t)0));
            }
            printf("\n");
        } else {
            return 2;
        }
    }
    t.release();
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
