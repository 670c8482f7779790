// annotate_walk.cpp — host model of zsw_annotate_batch: zoe_amd/csrc/zsw_annotate.hpp compiled for the host, the same text the
// kernel (zoe_amd/csrc/zsw_annotate.hip) compiles. The walk — op classes, cursors, gap cost, error order, the add_state / add_ciglet
// merge, the sweeps of ANN_G columns and the run extraction from their match masks — runs here exactly as on the device; the Io
// behind it loops over the ANN_G lanes where the kernel has a wavefront (one column per lane, a ballot, a reduction, one run per
// lane). What this model does not cover: the kernel's own Io (WaveIo), its loads from LDS, the launches and the entry point's
// argument checks; tests/test_gpu_annotate.py compares those with tests/annotate_ref.py on the device.
//
// Every array sits in a heap block of exactly its size, so that -fsanitize=address,undefined sees any index the walk derives from
// a malformed record (tests/test_annotate_model.py runs the malformed records through such a build).
//
// usage: annotate_walk <cases.txt>   (format: read_cases below; one result line per case on stdout)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../zoe_amd/csrc/zsw_annotate.hpp"

using namespace zsw::ann;

namespace {

struct Scoring {
    int S = 0, gap_open = 0, gap_extend = 0;  // positive magnitudes, as the library keeps them
    std::vector<uint8_t> im;
    std::vector<int32_t> w;
};

struct HostIo {
    const uint8_t *qseq, *rseq;
    bool q_is_read, shared, residues;
    const Scoring* sc;
    const uint32_t* inc;
    const uint8_t* op;
    uint32_t* out_inc;
    uint8_t* out_op;
    uint32_t out_n;
    int32_t sum[ANN_G] = {};

    void ciglet(uint32_t k, uint32_t* i, uint8_t* o) const {
        *i = inc[k];
        *o = op[k];
    }
    uint64_t sweep(uint64_t q, uint64_t r, int nv) {
        uint64_t mask = 0;
        for (int lane = 0; lane < ANN_G; ++lane) {
            if (lane >= nv) continue;
            const uint8_t qb = qseq[q + lane], rb = rseq[r + lane];
            const int qi = sc->im[qb], ri = sc->im[rb];
            const bool eq = residues ? qi == ri : qb == rb;
            const int read_i = q_is_read ? qi : ri, seq_i = q_is_read ? ri : qi;
            sum[lane] += shared ? sc->w[read_i * sc->S + seq_i] : sc->w[seq_i * sc->S + read_i];
            if (eq) mask |= 1ull << lane;
        }
        return mask;
    }
    int64_t column_score() const {
        int32_t v = 0;
        for (int lane = 0; lane < ANN_G; ++lane) v += sum[lane];
        return v;
    }
    void emit_one(uint32_t pos, uint32_t i, uint8_t o) const {
        if (pos < out_n) {
            out_inc[pos] = i;
            out_op[pos] = o;
        }
    }
    void emit_runs(uint64_t starts, uint64_t mask, uint32_t pos) const {
        for (int lane = 0; lane < ANN_G; ++lane) {
            uint32_t i, rank;
            uint8_t o;
            if (run_of_lane(starts, mask, lane, &i, &o, &rank) && (uint64_t)pos + rank < out_n) {
                out_inc[pos + rank] = i;
                out_op[pos + rank] = o;
            }
        }
    }
};

// exactly n bytes on the heap (n == 0: a block of one byte that nothing may read is still a valid pointer)
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

// One read as the kernel treats it: the count launch, then (for an annotated read) the write launch.
void run_case(const Scoring& sc, int flags, int status, const std::vector<uint8_t>& read, const std::vector<uint8_t>& seq, const Rec& rec,
              const std::vector<uint32_t>& inc_v, const std::vector<uint8_t>& op_v) {
    uint8_t *rd = exact(read), *sq = exact(seq), *op = exact(op_v);
    uint32_t* inc = exact(inc_v);
    const bool read_is_ref = (flags & F_READ_IS_REF) != 0;
    const uint32_t len = (uint32_t)read.size(), seq_len = (uint32_t)seq.size();
    const bool ok = record_ok(rec, inc_v.size(), read_is_ref ? len : seq_len, read_is_ref ? seq_len : len);
    Stats s{};
    s.path_status = status != 0 ? P_NO_ALIGNMENT : ok ? P_OK : P_BAD_RECORD;
    uint32_t nv = 0;
    std::vector<uint32_t> out_inc;
    std::vector<uint8_t> out_op;
    if (s.path_status == P_OK) {
        HostIo io;
        io.qseq = read_is_ref ? sq : rd;
        io.rseq = read_is_ref ? rd : sq;
        io.q_is_read = !read_is_ref;
        io.shared = (flags & F_SHARED) != 0;
        io.residues = (flags & F_MATCH_RESIDUES) != 0;
        io.sc = &sc;
        io.inc = inc + rec.ciglet_offset;
        io.op = op + rec.ciglet_offset;
        io.out_inc = nullptr;
        io.out_op = nullptr;
        io.out_n = 0;
        s = walk<false>(io, rec, sc.gap_open, sc.gap_extend, &nv);
        if (annotated(s.path_status)) {
            out_inc.assign(nv, 0xdeadbeefu);
            out_op.assign(nv, '?');
            uint32_t* oi = exact(out_inc);
            uint8_t* oo = exact(out_op);
            HostIo io2 = io;
            memset(io2.sum, 0, sizeof(io2.sum));
            io2.out_inc = oi;
            io2.out_op = oo;
            io2.out_n = nv;
            uint32_t nv2 = 0;
            const Stats s2 = walk<true>(io2, rec, sc.gap_open, sc.gap_extend, &nv2);
            if (nv2 != nv || memcmp(&s2, &s, sizeof(s))) {
                fprintf(stderr, "the write walk disagrees with the count walk\n");
                exit(3);
            }
            if (nv) {
                memcpy(out_inc.data(), oi, nv * 4);
                memcpy(out_op.data(), oo, nv);
            }
            free(oi);
            free(oo);
        }
    }
    printf("%u %u %u %u %u %u %d %u %u", s.matches, s.mismatches, s.ins_bases, s.del_bases, s.ins_runs, s.del_runs, s.path_score, s.path_status, nv);
    for (uint32_t k = 0; k < nv; ++k) printf(" %u %u", out_inc[k], (unsigned)out_op[k]);
    printf("\n");
    free(rd);
    free(sq);
    free(op);
    free(inc);
}

// scoring S gap_open gap_extend / 256 index-map entries / S * S weights (row-major), then any number of
//   seq <hex | ->                                      the context's sequence of the cases that follow
//   case flags status <read hex | -> score ref_start ref_end query_start query_end ref_len query_len n_ciglets ciglet_offset total
//        followed by `total` pairs "inc op" (op as a number): the whole ciglet arrays of the call
int read_cases(FILE* f) {
    Scoring sc;
    char word[64];
    if (fscanf(f, "%63s %d %d %d", word, &sc.S, &sc.gap_open, &sc.gap_extend) != 4 || strcmp(word, "scoring") || sc.S < 1 || sc.S > 32) return 2;
    sc.im.resize(256);
    sc.w.resize((size_t)sc.S * sc.S);
    for (auto& x : sc.im) {
        unsigned v;
        if (fscanf(f, "%u", &v) != 1 || v >= (unsigned)sc.S) return 2;
        x = (uint8_t)v;
    }
    for (auto& x : sc.w)
        if (fscanf(f, "%d", &x) != 1) return 2;
    std::vector<uint8_t> seq;
    std::string buf;
    while (fscanf(f, "%63s", word) == 1) {
        auto token = [&]() {
            buf.clear();
            int c;
            while ((c = fgetc(f)) != EOF && (c == ' ' || c == '\n')) {}
            for (; c != EOF && c != ' ' && c != '\n'; c = fgetc(f)) buf.push_back((char)c);
            return buf.c_str();
        };
        if (!strcmp(word, "seq")) {
            seq = unhex(token());
        } else if (!strcmp(word, "case")) {
            int flags, status;
            if (fscanf(f, "%d %d", &flags, &status) != 2) return 2;
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
            run_case(sc, flags, status, read, seq, rec, inc, op);
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
