// zoe_sw.hpp — header-only C++ mirror of the reference's interface over the C ABI (zoe_sw.h).
//
// Names follow the reference (file:line in the reference checkout):
//   zoe::ByteIndexMap / DNA_PROFILE_MAP     src/data/constants/mappings/byte_index.rs:231-358, dna.rs:177-178
//   zoe::WeightMatrix                       src/data/matrices/mod.rs:230-546
//   zoe::ProfileError                       src/alignment/errors.rs:6-15
//   zoe::MaybeAligned / Alignment           src/alignment/types/output.rs:18-25, 264-279
//   zoe::StripedProfileBatch                src/alignment/profile.rs:198-552 (one StripedProfile<T,N,S> per read of a batch)
//   zoe::LocalProfilesBatch                 src/alignment/profile_set.rs:382-483 (one LocalProfiles per read of a batch)
// Host-memory batches; one zoe::GpuContext per GPU.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "zoe_sw.h"

namespace zoe {

struct ProfileError : std::runtime_error {
    int code;  // 1 EmptySequence, 2 GapOpenOutOfRange, 3 GapExtendOutOfRange, 4 BadGapWeights
    explicit ProfileError(int c)
        : std::runtime_error(c == 1 ? "EmptySequence" : c == 2 ? "GapOpenOutOfRange" : c == 3 ? "GapExtendOutOfRange" : "BadGapWeights"), code(c) {}
};
struct GpuError : std::runtime_error {
    int code;
    GpuError(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

struct ByteIndexMap {
    std::array<uint8_t, 256> index_map{};
    std::string byte_keys;
    static ByteIndexMap make(const std::string& keys, char catch_all, bool ignore_case) {
        ByteIndexMap m;
        auto up = [](unsigned char c) -> unsigned char { return (c >= 'a' && c <= 'z') ? c - 32 : c; };
        auto lo = [](unsigned char c) -> unsigned char { return (c >= 'A' && c <= 'Z') ? c + 32 : c; };
        m.byte_keys = keys;
        int ca = -1;
        for (size_t i = 0; i < keys.size(); ++i)
            if ((ignore_case ? up(keys[i]) : (unsigned char)keys[i]) == (ignore_case ? up(catch_all) : (unsigned char)catch_all)) ca = (int)i;
        if (ca < 0) throw std::invalid_argument("The catch_all must be present in the byte_keys.");
        m.index_map.fill((uint8_t)ca);
        for (size_t i = 0; i < keys.size(); ++i) {
            if (ignore_case) {
                m.index_map[up(keys[i])] = (uint8_t)i;
                m.index_map[lo(keys[i])] = (uint8_t)i;
            } else {
                m.index_map[(unsigned char)keys[i]] = (uint8_t)i;
            }
        }
        return m;
    }
    ByteIndexMap add_synonym_ignore_case(char new_key, char previous_key) const {
        ByteIndexMap m = *this;
        const uint8_t idx = m.index_map[(unsigned char)previous_key];
        unsigned char c = (unsigned char)new_key;
        m.index_map[(c >= 'a' && c <= 'z') ? c - 32 : c] = idx;
        m.index_map[(c >= 'A' && c <= 'Z') ? c + 32 : c] = idx;
        return m;
    }
    size_t len() const { return byte_keys.size(); }
    size_t to_index(uint8_t b) const { return index_map[b]; }
};

inline const ByteIndexMap& DNA_PROFILE_MAP() {
    static const ByteIndexMap m = ByteIndexMap::make("ACGTN", 'N', true).add_synonym_ignore_case('U', 'T');
    return m;
}

struct WeightMatrix {
    std::vector<int8_t> weights;  // [ref residue * S + query residue]
    const ByteIndexMap* mapping;
    int S;
    // WeightMatrix::new (matrices/mod.rs:358-399); ignoring < 0: none
    static WeightMatrix make(const ByteIndexMap& map, int8_t matching, int8_t mismatch, int ignoring) {
        WeightMatrix w;
        w.mapping = &map;
        w.S = (int)map.len();
        w.weights.assign((size_t)w.S * w.S, 0);
        const int skip = ignoring >= 0 ? (int)map.to_index((uint8_t)ignoring) : -1;
        for (int i = 0; i < w.S; ++i)
            for (int j = 0; j < w.S; ++j)
                if (!(skip >= 0 && (skip == i || skip == j))) w.weights[(size_t)i * w.S + j] = i == j ? matching : mismatch;
        return w;
    }
    static WeightMatrix new_dna_matrix(int8_t matching, int8_t mismatch, int ignoring) {
        return make(DNA_PROFILE_MAP(), matching, mismatch, ignoring);
    }
};

// BelowMinScore: only under GpuContext::set_min_score(t > 0) — the read scores less than t; it has no value, like an Unmapped one
enum class Status : uint8_t { Some = 0, Overflowed = 1, Unmapped = 2, Empty = 3, BelowMinScore = 4 };

template <typename T> struct MaybeAligned {
    Status status = Status::Unmapped;
    T value{};
    bool is_some() const { return status == Status::Some; }
    const T& unwrap() const {
        if (status == Status::Overflowed) throw std::runtime_error("Alignment score overflowed!");
        if (status != Status::Some) throw std::runtime_error("Sequence could not be mapped!");
        return value;
    }
};

struct Ciglet {
    size_t inc;
    uint8_t op;
};
struct Alignment {
    uint32_t score = 0;
    size_t ref_start = 0, ref_end = 0, query_start = 0, query_end = 0, ref_len = 0, query_len = 0;
    std::vector<Ciglet> states;
    std::string cigar() const {
        std::string s;
        for (auto& c : states) {
            s += std::to_string(c.inc);
            s.push_back((char)c.op);
        }
        return s;
    }
    // AlignmentStates::add_ciglet (types/state.rs:142-152): equal neighbours merge, an inc of 0 adds nothing
    static void add_ciglet(std::vector<Ciglet>& states, size_t inc, uint8_t op) {
        if (!inc) return;
        if (!states.empty() && states.back().op == op) states.back().inc += inc;
        else states.push_back({inc, op});
    }
    // Alignment::to_verbose_sequence_matching (types/output.rs:456-479) on the host, one alignment at a time: M becomes = where the
    // bytes are equal and X elsewhere; `reference` is the whole reference. Throws where the reference panics (a path that leaves a
    // sequence). A batch goes through annotate() of the profile classes, which does this on the GPU.
    Alignment to_verbose_sequence_matching(const std::string& reference, const std::string& query) const {
        Alignment out = *this;
        out.states.clear();
        size_t r = ref_start, q = 0;
        for (const Ciglet& c : states) {
            if (c.op == 'M') {
                if (r + c.inc > reference.size() || q + c.inc > query.size()) throw std::out_of_range("to_verbose_sequence_matching: the alignment leaves a sequence");
                for (size_t k = 0; k < c.inc; ++k) add_ciglet(out.states, 1, query[q + k] == reference[r + k] ? '=' : 'X');
            } else {
                add_ciglet(out.states, c.inc, c.op);
            }
            if (c.op == 'M' || c.op == '=' || c.op == 'X' || c.op == 'I' || c.op == 'S') q += c.inc;
            if (c.op == 'M' || c.op == '=' || c.op == 'X' || c.op == 'D' || c.op == 'N') r += c.inc;
        }
        return out;
    }
};

// zsw_alignment_stats per read, and (if asked for) the alignments of Alignment::to_verbose_sequence_matching: what annotate() of the
// profile classes returns (zsw_annotate_batch)
struct Annotation {
    std::vector<zsw_alignment_stats> stats;
    std::vector<MaybeAligned<Alignment>> verbose;  // empty without `verbose`
    // the NM tag of SAM: mismatches + inserted + deleted bases
    uint32_t nm(size_t i) const { return stats[i].mismatches + stats[i].ins_bases + stats[i].del_bases; }
};

// What pileup() of the profile classes returns (zsw_pileup_batch): per position of the sequence the reads were aligned to, how often a
// read byte of each bin (A, C, G, T/U, N, gap, other IUPAC, invalid) stood opposite it; with `insertions`, per position the
// insertion runs and bases in front of it (len + 1 entries). Passed back in, a later call adds to it.
struct Pileup {
    std::vector<zsw_site_counts> counts;
    std::vector<zsw_site_insertions> insertions;  // empty without `insertions`
    uint64_t n_bad = 0;                           // records that are no alignments of their reads to the sequence: they count nothing
};

// What GpuContext::parse_fastq returns (zsw_fastq_parse_batch): the records in front of the first malformed one, and the report
// (ZSW_FASTQ_INFO_*: records, bases, name bytes, consumed, error, its record and offset, min / max length)
struct FastqRecords {
    std::vector<std::string> names, reads, quals;
    uint64_t report[ZSW_FASTQ_INFO_WORDS] = {};
    uint64_t error() const { return report[ZSW_FASTQ_INFO_ERROR]; }
};

// What GpuContext::parse_fasta returns (zsw_fasta_parse_batch): the records in front of the first malformed one — names as the raw
// header bytes, sequences with their line breaks removed — and the report (ZSW_FASTA_INFO_*, the words of ZSW_FASTQ_INFO_*)
struct FastaRecords {
    std::vector<std::string> names, sequences;
    uint64_t report[ZSW_FASTA_INFO_WORDS] = {};
    uint64_t error() const { return report[ZSW_FASTA_INFO_ERROR]; }
    // the reader's words for a ZSW_FASTA_* code
    static const char* error_text(uint64_t code) {
        switch (code) {
            case ZSW_FASTA_NO_DATA: return "No FASTA data found!";
            case ZSW_FASTA_MISSING_GT: return "The FASTA file must start with a '>' symbol!";
            case ZSW_FASTA_MISSING_HEADER: return "Missing FASTA header!";
            case ZSW_FASTA_GT_IN_HEADER: return "FASTA records must start with the '>' symbol on a newline, and no other '>' symbols can occur in a header!";
            case ZSW_FASTA_MISSING_SEQUENCE: return "Missing FASTA sequence!";
            case ZSW_FASTA_GT_IN_SEQUENCE: return "FASTA records must start with the '>' symbol on a newline, and no other '>' symbols can occur in a sequence!";
        }
        return "";
    }
};

// What GpuContext::parse_sam returns (zsw_sam_parse_batch): the data lines in front of the first malformed line — names, the reads
// as aligned (SEQ), qualities, the alignments as SamData::to_alignment builds them (Status::Unmapped for unmapped lines, lines of
// another RNAME and lines with a conversion code), FLAG & 16 per record, the rest of each line — and the report (ZSW_SAMTEXT_INFO_*)
struct SamRecords {
    std::vector<std::string> names, reads, quals;
    std::vector<MaybeAligned<Alignment>> alns;
    std::vector<uint8_t> strands;
    std::vector<zsw_sam_parsed> parsed;
    uint64_t report[ZSW_SAMTEXT_INFO_WORDS] = {};
    uint64_t error() const { return report[ZSW_SAMTEXT_INFO_ERROR]; }
    // the reader's words for a ZSW_SAMTEXT_* code
    static const char* error_text(uint64_t code) {
        switch (code) {
            case ZSW_SAMTEXT_INVALID_UTF8: return "the line is not valid UTF-8";
            case ZSW_SAMTEXT_TOO_FEW_FIELDS: return "SAM file did not have at least 11 fields";
            case ZSW_SAMTEXT_INVALID_FLAG: return "invalid SAM bit flag";
            case ZSW_SAMTEXT_INVALID_POS: return "invalid SAM reference position";
            case ZSW_SAMTEXT_INVALID_MAPQ: return "invalid SAM mapq";
            case ZSW_SAMTEXT_INVALID_QUALITY: return "invalid quality score byte";
            default: return "no error";
        }
    }
};

class GpuContext {
  public:
    explicit GpuContext(int device = 0) {
        zsw_error e = zsw_create(device, &ctx_);
        if (e != ZSW_OK) throw GpuError(e, std::string("zsw_create: ") + zsw_last_error_string(nullptr));
    }
    ~GpuContext() { zsw_destroy(ctx_); }
    GpuContext(const GpuContext&) = delete;
    GpuContext& operator=(const GpuContext&) = delete;
    zsw_context* raw() const { return ctx_; }
    // zsw_set_option(ZSW_OPTION_EXACT_PRUNING): the exact column-pruned first pass (same results for every input)
    void set_exact_pruning(bool on) { check(zsw_set_option(ctx_, ZSW_OPTION_EXACT_PRUNING, on ? 1 : 0)); }
    // zsw_set_option(ZSW_OPTION_MIN_SCORE): reads that score less than t come back as Status::BelowMinScore, settled by the seeded
    // pass's upper bounds where those suffice; 0 = off. Score, ends, ranges and 3-pass calls (zoe_sw.h); the others throw while t > 0.
    void set_min_score(uint32_t t) { check(zsw_set_option(ctx_, ZSW_OPTION_MIN_SCORE, (int64_t)t)); }
    // zsw_min_score_counts of the last covered call: settled below by the whole-read bound, a band bound, the exact score; in total
    std::vector<uint64_t> min_score_counts() const {
        std::vector<uint64_t> c(4, 0);
        check(zsw_min_score_counts(ctx_, c.data()));
        return c;
    }
    // zsw_set_panel: the members of a reference panel (1 .. ZSW_PANEL_MAX_REFS non-empty sequences), independent of the reference
    void set_panel(const std::vector<std::string>& members) {
        std::vector<uint8_t> seqs;
        std::vector<uint64_t> offsets(1, 0);
        for (const std::string& m : members) {
            seqs.insert(seqs.end(), m.begin(), m.end());
            offsets.push_back(seqs.size());
        }
        seqs.push_back(0);
        check(zsw_set_panel(ctx_, seqs.data(), offsets.data(), (uint32_t)members.size(), ZSW_MEM_HOST));
    }
    // zsw_panel_counts of the last panel call: reads settled after one score, pairs scored in the first / second round, reads
    // scored against every member
    std::vector<uint64_t> panel_counts() const {
        std::vector<uint64_t> c(4, 0);
        check(zsw_panel_counts(ctx_, c.data()));
        return c;
    }
    void check(zsw_error e) const {
        if (e == ZSW_OK) return;
        if (e >= 1 && e <= 4) throw ProfileError(e);
        throw GpuError(e, zsw_last_error_string(ctx_));
    }
    // zsw_annotate_batch over alignments that a call on `reads` (a host batch) returned, with scoring and the sequence the flags
    // name set on this context: the records are flattened again, annotated on the GPU, and rebuilt. flags: ZSW_ANNOTATE_*.
    Annotation annotate(const zsw_batch& reads, int flags, const std::vector<MaybeAligned<Alignment>>& alns, bool verbose) const {
        const size_t n = alns.size();
        if (n != reads.n_reads) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one alignment per read");
        std::vector<zsw_alignment> rec;
        std::vector<uint8_t> status;
        std::vector<uint32_t> inc;
        std::vector<uint8_t> op;
        flatten(alns, rec, status, inc, op);
        Annotation out;
        out.stats.resize(n);
        if (!verbose) {
            check(zsw_annotate_batch(ctx_, &reads, flags, rec.data(), status.data(), inc.data(), op.data(), inc.size(), out.stats.data(), nullptr, nullptr, nullptr,
                                     0, nullptr, nullptr));
            return out;
        }
        std::vector<zsw_alignment> vrec(n);
        std::vector<uint32_t> vinc(2 * inc.size() + 64);
        std::vector<uint8_t> vop(vinc.size());
        uint64_t total = 0;
        auto call = [&]() {
            return zsw_annotate_batch(ctx_, &reads, flags, rec.data(), status.data(), inc.data(), op.data(), inc.size(), out.stats.data(), vrec.data(), vinc.data(),
                                      vop.data(), (uint64_t)vinc.size(), &total, nullptr);
        };
        zsw_error e = call();
        if (e == ZSW_ERR_INVALID_ARGUMENT && total > vinc.size()) {
            vinc.resize(total);
            vop.resize(total);
            e = call();
        }
        check(e);
        out.verbose = alns;
        for (size_t i = 0; i < n; ++i) {
            out.verbose[i].value.states.clear();
            for (uint32_t k = 0; k < vrec[i].n_ciglets; ++k) out.verbose[i].value.states.push_back({vinc[vrec[i].ciglet_offset + k], vop[vrec[i].ciglet_offset + k]});
        }
        return out;
    }
    // zsw_pileup_batch over alignments that a call on `reads` (a host batch: the reads as aligned) returned, with the sequence the
    // flags name (len bases) set on this context. flags: ZSW_ANNOTATE_READ_IS_REF / ZSW_ANNOTATE_SHARED. `into`: the table of an
    // earlier call over the same sequence, which is added to.
    Pileup pileup(const zsw_batch& reads, int flags, const std::vector<MaybeAligned<Alignment>>& alns, size_t len, bool insertions, const Pileup* into = nullptr) const {
        if (alns.size() != reads.n_reads) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one alignment per read");
        std::vector<zsw_alignment> rec;
        std::vector<uint8_t> status;
        std::vector<uint32_t> inc;
        std::vector<uint8_t> op;
        flatten(alns, rec, status, inc, op);
        Pileup out;
        if (into) out = *into;
        out.counts.resize(len);
        if (insertions) out.insertions.resize(len + 1);
        uint64_t n_bad = 0;
        check(zsw_pileup_batch(ctx_, &reads, flags, rec.data(), status.data(), inc.data(), op.data(), inc.size(), out.counts.data(),
                               insertions ? out.insertions.data() : nullptr, &n_bad, nullptr));
        out.n_bad += n_bad;
        return out;
    }
    // zsw_consensus_from_counts: CreateConsensus::plurality_acgtn of a table of pileup(); fallback: positions without any A C G T N
    // count keep its byte (ZSW_CONSENSUS_KEEP_UNCOVERED)
    std::string plurality_acgtn(const std::vector<zsw_site_counts>& counts, const std::string* fallback = nullptr) const {
        if (fallback && fallback->size() != counts.size()) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one fallback byte per position");
        std::string out(counts.size(), 'A');
        check(zsw_consensus_from_counts(ctx_, counts.data(), counts.size(), ZSW_MEM_HOST, fallback ? ZSW_CONSENSUS_KEEP_UNCOVERED : 0,
                                        fallback ? reinterpret_cast<const uint8_t*>(fallback->data()) : nullptr, reinterpret_cast<uint8_t*>(&out[0]), nullptr));
        return out;
    }
    // zsw_sam_batch over alignments that a call on `reads` (a host batch: the reads as aligned) returned: the SAM body, one line per
    // read, formatted on the GPU. fields: names, qualities, strands, stats, RNAME and MAPQ as the C ABI takes them (host arrays).
    std::string sam_text(const zsw_batch& reads, const zsw_sam_fields& fields, int flags, const std::vector<MaybeAligned<Alignment>>& alns) const {
        if (alns.size() != reads.n_reads) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one alignment per read");
        std::vector<zsw_alignment> rec;
        std::vector<uint8_t> status;
        std::vector<uint32_t> inc;
        std::vector<uint8_t> op;
        flatten(alns, rec, status, inc, op);
        uint64_t total = 0, n_bad = 0;
        check(zsw_sam_batch(ctx_, &reads, &fields, flags, rec.data(), status.data(), inc.data(), op.data(), inc.size(), nullptr, 0, &total, nullptr, &n_bad, nullptr));
        std::string text(total, '\0');
        if (total)
            check(zsw_sam_batch(ctx_, &reads, &fields, flags, rec.data(), status.data(), inc.data(), op.data(), inc.size(), (uint8_t*)&text[0], total, &total, nullptr,
                                &n_bad, nullptr));
        return text;
    }
    // zsw_fastq_parse_batch over the bytes of a FASTQ buffer (host memory): the records FastQReader yields in front of its first
    // error, as names, reads and qualities, and the report. last: the buffer ends the file (ZSW_FASTQ_FINAL); without it only the
    // records whose four lines are all terminated are parsed and report[ZSW_FASTQ_INFO_CONSUMED] says where the rest begins.
    // name_to_blank: names end in front of the first space or tab. A malformed record does not throw: report[ZSW_FASTQ_INFO_ERROR].
    FastqRecords parse_fastq(const std::string& text, bool last = true, bool name_to_blank = false) const {
        const uint64_t n = text.size(), base_cap = n / 2, name_cap = n, record_cap = n / 8 + 1;  // the bounds that always suffice
        std::vector<uint8_t> bases(base_cap + 1), quals(base_cap + 1), qnames(name_cap + 1);
        std::vector<uint64_t> off(record_cap + 1), noff(record_cap + 1);
        FastqRecords out;
        check(zsw_fastq_parse_batch(ctx_, reinterpret_cast<const uint8_t*>(text.data()), n, ZSW_MEM_HOST, (last ? ZSW_FASTQ_FINAL : 0) | (name_to_blank ? ZSW_FASTQ_NAME_TO_BLANK : 0),
                                    bases.data(), quals.data(), base_cap, off.data(), qnames.data(), name_cap, noff.data(), record_cap, out.report, nullptr));
        const size_t records = (size_t)out.report[ZSW_FASTQ_INFO_RECORDS];
        out.names.reserve(records);
        out.reads.reserve(records);
        out.quals.reserve(records);
        for (size_t i = 0; i < records; ++i) {
            out.names.emplace_back(qnames.begin() + noff[i], qnames.begin() + noff[i + 1]);
            out.reads.emplace_back(bases.begin() + off[i], bases.begin() + off[i + 1]);
            out.quals.emplace_back(quals.begin() + off[i], quals.begin() + off[i + 1]);
        }
        return out;
    }
    // zsw_fasta_parse_batch over the bytes of a FASTA buffer (host memory): the records FastaReader yields in front of its first
    // error, as names and sequences, and the report. last: the buffer ends the file (ZSW_FASTA_FINAL); without it the record at the
    // last '>' is left for the next call, which starts at report[ZSW_FASTA_INFO_CONSUMED] with `continued`. name_to_blank: names end
    // in front of the first space or tab. A malformed record does not throw: report[ZSW_FASTA_INFO_ERROR].
    FastaRecords parse_fasta(const std::string& text, bool last = true, bool name_to_blank = false, bool continued = false) const {
        const uint64_t n = text.size(), base_cap = n, name_cap = n, record_cap = n / 4 + 1;  // the bounds that always suffice
        std::vector<uint8_t> bases(base_cap + 1), names(name_cap + 1);
        std::vector<uint64_t> off(record_cap + 1), noff(record_cap + 1);
        FastaRecords out;
        const int flags = (last ? ZSW_FASTA_FINAL : 0) | (name_to_blank ? ZSW_FASTA_NAME_TO_BLANK : 0) | (continued ? ZSW_FASTA_CONTINUED : 0);
        check(zsw_fasta_parse_batch(ctx_, reinterpret_cast<const uint8_t*>(text.data()), n, ZSW_MEM_HOST, flags, bases.data(), base_cap, off.data(), names.data(), name_cap,
                                    noff.data(), record_cap, out.report, nullptr));
        const size_t records = (size_t)out.report[ZSW_FASTA_INFO_RECORDS];
        out.names.reserve(records);
        out.sequences.reserve(records);
        for (size_t i = 0; i < records; ++i) {
            out.names.emplace_back(names.begin() + noff[i], names.begin() + noff[i + 1]);
            out.sequences.emplace_back(bases.begin() + off[i], bases.begin() + off[i + 1]);
        }
        return out;
    }
    // zsw_sam_parse_batch over SAM text (host memory): a sizing call, then the call with arrays of the reported sizes. last: the
    // buffer ends the file (ZSW_SAMTEXT_FINAL); otherwise report[ZSW_SAMTEXT_INFO_CONSUMED] says where the rest begins. qual_forward:
    // the QUAL of a FLAG 16 line is stored back to front, as sam_text() takes it. rname (empty: none): lines of another RNAME come
    // back unmapped. ref_len: the ref_len of every alignment. A malformed line does not throw: report[ZSW_SAMTEXT_INFO_ERROR].
    SamRecords parse_sam(const std::string& text, bool last = true, bool qual_forward = true, const std::string& rname = std::string(), uint32_t ref_len = 0) const {
        const int flags = (last ? ZSW_SAMTEXT_FINAL : 0) | (qual_forward ? ZSW_SAMTEXT_QUAL_FORWARD : 0);
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(text.data());
        const char* rn = rname.empty() ? nullptr : rname.data();
        SamRecords out;
        zsw_sam_parse_out o{};
        check(zsw_sam_parse_batch(ctx_, bytes, text.size(), ZSW_MEM_HOST, flags, rn, (uint32_t)rname.size(), ref_len, &o, out.report, nullptr));
        const size_t records = (size_t)out.report[ZSW_SAMTEXT_INFO_RECORDS], n_bases = (size_t)out.report[ZSW_SAMTEXT_INFO_BASES];
        const size_t n_names = (size_t)out.report[ZSW_SAMTEXT_INFO_NAME_BYTES], n_ciglets = (size_t)out.report[ZSW_SAMTEXT_INFO_CIGLETS];
        std::vector<uint8_t> bases(n_bases + 1), quals(n_bases + 1), qnames(n_names + 1), status(records + 1), op(n_ciglets + 1);
        std::vector<uint64_t> off(records + 1), noff(records + 1);
        std::vector<zsw_alignment> aln(records + 1);
        std::vector<uint32_t> inc(n_ciglets + 1);
        out.strands.assign(records + 1, 0);
        out.parsed.assign(records + 1, zsw_sam_parsed{});
        o.bases = bases.data(), o.quals = quals.data(), o.base_cap = n_bases, o.offsets = off.data();
        o.qnames = qnames.data(), o.name_cap = n_names, o.qname_offsets = noff.data();
        o.aln = aln.data(), o.status = status.data(), o.inc = inc.data(), o.op = op.data(), o.ciglet_cap = n_ciglets;
        o.strand = out.strands.data(), o.parsed = out.parsed.data(), o.record_cap = records;
        check(zsw_sam_parse_batch(ctx_, bytes, text.size(), ZSW_MEM_HOST, flags, rn, (uint32_t)rname.size(), ref_len, &o, out.report, nullptr));
        out.strands.resize(records);
        out.parsed.resize(records);
        out.alns.resize(records);
        for (size_t i = 0; i < records; ++i) {
            out.names.emplace_back(qnames.begin() + noff[i], qnames.begin() + noff[i + 1]);
            out.reads.emplace_back(bases.begin() + off[i], bases.begin() + off[i + 1]);
            out.quals.emplace_back(quals.begin() + off[i], quals.begin() + off[i + 1]);
            out.alns[i].status = (Status)status[i];
            if (status[i] != ZSW_STATUS_SOME) continue;
            Alignment& a = out.alns[i].value;
            a.score = aln[i].score;
            a.ref_start = aln[i].ref_start, a.ref_end = aln[i].ref_end, a.query_start = aln[i].query_start, a.query_end = aln[i].query_end;
            a.ref_len = aln[i].ref_len, a.query_len = aln[i].query_len;
            for (uint32_t k = 0; k < aln[i].n_ciglets; ++k) a.states.push_back({inc[aln[i].ciglet_offset + k], op[aln[i].ciglet_offset + k]});
        }
        return out;
    }

  private:
    // Alignments -> the records and ciglet arrays of the C ABI
    static void flatten(const std::vector<MaybeAligned<Alignment>>& alns, std::vector<zsw_alignment>& rec, std::vector<uint8_t>& status, std::vector<uint32_t>& inc,
                        std::vector<uint8_t>& op) {
        const size_t n = alns.size();
        rec.resize(n);
        status.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const Alignment& a = alns[i].value;
            status[i] = (uint8_t)alns[i].status;
            rec[i] = zsw_alignment{a.score, (uint32_t)a.ref_start, (uint32_t)a.ref_end, (uint32_t)a.query_start, (uint32_t)a.query_end, (uint32_t)a.ref_len,
                                   (uint32_t)a.query_len, (uint32_t)a.states.size(), (uint64_t)inc.size()};
            for (const Ciglet& c : a.states) {
                if (c.inc > 0xffffffffull) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "a ciglet beyond 32 bits");
                inc.push_back((uint32_t)c.inc);
                op.push_back(c.op);
            }
        }
    }
    zsw_context* ctx_ = nullptr;
};

// ScoreEnds / ScoreAndRanges (src/alignment/types/output.rs:201-219); ranges are 0-based half-open
struct ScoreEnds {
    uint32_t score = 0;
    size_t ref_end = 0, query_end = 0;
};
struct ScoreAndRanges {
    uint32_t score = 0;
    size_t ref_start = 0, ref_end = 0, query_start = 0, query_end = 0;
};

// Reads of a batch (host memory) bound to one scoring scheme; the common part of the two profile mirrors below.
class ProfileBatchBase {
  public:
    size_t size() const { return offsets_.size() - 1; }

  protected:
    ProfileBatchBase(GpuContext& ctx, const std::vector<std::string>& reads, const WeightMatrix& matrix, int8_t gap_open, int8_t gap_extend)
        : ctx_(ctx) {
        offsets_.reserve(reads.size() + 1);
        offsets_.push_back(0);
        for (auto& r : reads) {
            if (r.empty()) throw ProfileError(1);  // validate_profile_args (profile.rs:32-44)
            bases_.insert(bases_.end(), r.begin(), r.end());
            offsets_.push_back(bases_.size());
        }
        ctx_.check(zsw_set_scoring(ctx_.raw(), matrix.weights.data(), matrix.S, matrix.mapping->index_map.data(), gap_open, gap_extend));
    }
    zsw_batch batch() const {
        zsw_batch b;
        b.bases = bases_.data();
        b.offsets = offsets_.data();
        b.fixed_len = 0;
        b.n_reads = offsets_.size() - 1;
        b.mem = ZSW_MEM_HOST;
        b.encoding = ZSW_ENCODING_BYTES;
        return b;
    }
    void set_reference(const std::string& reference) {
        ctx_.check(zsw_set_reference(ctx_.raw(), (const uint8_t*)reference.data(), reference.size(), ZSW_MEM_HOST));
    }
    // Runs an align-type entry point (growing the ciglet buffers once if the call asks for it) and rebuilds the Alignments.
    template <typename Call>
    std::vector<MaybeAligned<Alignment>> collect(Call call) {
        const size_t n = size();
        std::vector<zsw_alignment> aln(n);
        std::vector<uint8_t> status(n);
        std::vector<uint32_t> inc(16 * n + 64);
        std::vector<uint8_t> op(inc.size());
        uint64_t total = 0;
        zsw_error e = call(aln.data(), status.data(), inc.data(), op.data(), (uint64_t)inc.size(), &total);
        if (e == ZSW_ERR_INVALID_ARGUMENT && total > inc.size()) {
            inc.resize(total);
            op.resize(total);
            e = call(aln.data(), status.data(), inc.data(), op.data(), (uint64_t)inc.size(), &total);
        }
        ctx_.check(e);
        std::vector<MaybeAligned<Alignment>> out(n);
        for (size_t i = 0; i < n; ++i) {
            out[i].status = (Status)status[i];
            if (status[i] != 0) continue;
            Alignment& a = out[i].value;
            a.score = aln[i].score;
            a.ref_start = aln[i].ref_start;
            a.ref_end = aln[i].ref_end;
            a.query_start = aln[i].query_start;
            a.query_end = aln[i].query_end;
            a.ref_len = aln[i].ref_len;
            a.query_len = aln[i].query_len;
            for (uint32_t k = 0; k < aln[i].n_ciglets; ++k)
                a.states.push_back({inc[aln[i].ciglet_offset + k], op[aln[i].ciglet_offset + k]});
        }
        return out;
    }
    GpuContext& ctx_;
    std::vector<uint8_t> bases_;
    std::vector<uint64_t> offsets_;

  public:
    // zsw_annotate_batch over the alignments `alns` that one of this batch's alignment calls returned for `seq` (with the same
    // seq_is_query): counts, sw_score_from_path and, with `verbose`, the = / X CIGARs. residues: a column matches when the index map
    // sends both bytes to one residue (default: equal bytes, as the reference). strand: the strands of a strand-aware call, whose
    // alignments are annotated against the reads as aligned (zsw_orient_batch).
    Annotation annotate(const std::vector<MaybeAligned<Alignment>>& alns, const std::string& seq, bool seq_is_query = false, bool residues = false,
                        bool verbose = true, const std::vector<uint8_t>* strand = nullptr) {
        set_reference(seq);
        zsw_batch b = batch();
        std::vector<uint8_t> oriented;
        if (strand) {
            if (strand->size() != size()) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one strand per read");
            oriented.resize(bases_.size());
            ctx_.check(zsw_orient_batch(ctx_.raw(), &b, strand->data(), oriented.data(), nullptr));
            b.bases = oriented.data();
        }
        return ctx_.annotate(b, (seq_is_query ? ZSW_ANNOTATE_READ_IS_REF : 0) | (residues ? ZSW_ANNOTATE_MATCH_RESIDUES : 0), alns, verbose);
    }
    // zsw_pileup_batch over the alignments `alns` that one of this batch's alignment calls returned for `seq` (with the same
    // seq_is_query): the table over `seq`. strand: the strands of a strand-aware call, whose alignments are piled up from the reads
    // as aligned (zsw_orient_batch). into: the table of an earlier call over the same `seq`, which is added to.
    // ctx.plurality_acgtn(pileup.counts) is the consensus.
    Pileup pileup(const std::vector<MaybeAligned<Alignment>>& alns, const std::string& seq, bool seq_is_query = false, bool insertions = false,
                  const std::vector<uint8_t>* strand = nullptr, const Pileup* into = nullptr) {
        set_reference(seq);
        zsw_batch b = batch();
        std::vector<uint8_t> oriented;
        if (strand) {
            if (strand->size() != size()) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one strand per read");
            oriented.resize(bases_.size());
            ctx_.check(zsw_orient_batch(ctx_.raw(), &b, strand->data(), oriented.data(), nullptr));
            b.bases = oriented.data();
        }
        return ctx_.pileup(b, seq_is_query ? ZSW_ANNOTATE_READ_IS_REF : 0, alns, seq.size(), insertions, into);
    }
    // zsw_sam_batch: the SAM body for the alignments `alns` of this batch (those of an alignment call, or Annotation::verbose for
    // = / X CIGARs), one line per read in read order, as `SamData::from_alignment(..)` / `SamData::unmapped(..)` print them — without
    // the @HD / @SQ header. names: QNAME per read (empty vector: "*"); quals: the qualities as read, one string of the read's length
    // per read (empty vector: "*"); strands: of a strand-aware call — FLAG 16, SEQ reverse complemented (zsw_orient_batch) and QUAL
    // reversed for strand 1; annotation: its stats give NM:i: on mapped lines; omit_seq: SEQ "*".
    std::string sam_text(const std::vector<MaybeAligned<Alignment>>& alns, const std::vector<std::string>& names, const std::vector<std::string>& quals,
                         const std::string& rname, uint32_t mapq = 255, const std::vector<uint8_t>* strands = nullptr, const Annotation* annotation = nullptr,
                         bool omit_seq = false) {
        const size_t n = size();
        if ((!names.empty() && names.size() != n) || (!quals.empty() && quals.size() != n) || (strands && strands->size() != n) ||
            (annotation && annotation->stats.size() != n))
            throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one name, quality string, strand and stats entry per read");
        zsw_batch b = batch();
        std::vector<uint8_t> oriented, name_bytes, qual_bytes;
        std::vector<uint64_t> name_offsets;
        if (strands) {
            oriented.resize(bases_.size());
            ctx_.check(zsw_orient_batch(ctx_.raw(), &b, strands->data(), oriented.data(), nullptr));
            b.bases = oriented.data();
        }
        zsw_sam_fields f{};
        if (!names.empty()) {
            name_offsets.push_back(0);
            for (auto& s : names) {
                name_bytes.insert(name_bytes.end(), s.begin(), s.end());
                name_offsets.push_back(name_bytes.size());
            }
            name_bytes.push_back(0);  // a valid pointer when every name is empty
            f.qnames = name_bytes.data();
            f.qname_offsets = name_offsets.data();
        }
        if (!quals.empty()) {
            qual_bytes.reserve(bases_.size());
            for (size_t i = 0; i < n; ++i) {
                if (quals[i].size() != offsets_[i + 1] - offsets_[i]) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "a quality string is as long as its read");
                qual_bytes.insert(qual_bytes.end(), quals[i].begin(), quals[i].end());
            }
            f.quals = qual_bytes.data();
        }
        f.strand = strands ? strands->data() : nullptr;
        f.stats = annotation ? annotation->stats.data() : nullptr;
        f.rname = rname.data();
        f.rname_len = (uint32_t)rname.size();
        f.mapq = mapq;
        return ctx_.sam_text(b, f, omit_seq ? ZSW_SAM_OMIT_SEQ : 0, alns);
    }
};

// `StripedProfile::<T, N, S>::new(read_i, &matrix, gap_open, gap_extend)` for every read of a batch (profile.rs:239-247).
// Unsigned T takes the signed matrix too: the library derives the bias the way to_biased_matrix does (matrices/mod.rs:452-491).
class StripedProfileBatch : public ProfileBatchBase {
  public:
    StripedProfileBatch(GpuContext& ctx, const std::vector<std::string>& reads, const WeightMatrix& matrix, int8_t gap_open,
                        int8_t gap_extend, zsw_int_type T, int N)
        : ProfileBatchBase(ctx, reads, matrix, gap_open, gap_extend), T_(T), N_(N) {}
    // profile.rs:440-446 -> sw_simd_score (striped.rs:65-142)
    std::vector<MaybeAligned<uint32_t>> sw_score(const std::string& reference) {
        set_reference(reference);
        const size_t n = size();
        zsw_batch b = batch();
        std::vector<uint32_t> score(n);
        std::vector<uint8_t> status(n);
        ctx_.check(zsw_score_batch(ctx_.raw(), &b, T_, N_, score.data(), status.data(), nullptr));
        std::vector<MaybeAligned<uint32_t>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], score[i]};
        return out;
    }
    // profile.rs:456-460 -> sw_simd_score_ends (striped.rs:153-162)
    std::vector<MaybeAligned<ScoreEnds>> sw_score_ends(const std::string& reference) {
        set_reference(reference);
        const size_t n = size();
        zsw_batch b = batch();
        std::vector<uint32_t> score(n), re(n), qe(n);
        std::vector<uint8_t> status(n);
        ctx_.check(zsw_score_ends_batch(ctx_.raw(), &b, T_, N_, score.data(), re.data(), qe.data(), status.data(), nullptr));
        std::vector<MaybeAligned<ScoreEnds>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], ScoreEnds{score[i], re[i], qe[i]}};
        return out;
    }
    // profile.rs:529-533 -> sw_simd_score_ranges (striped.rs:355-388)
    std::vector<MaybeAligned<ScoreAndRanges>> sw_score_ranges(const std::string& reference) {
        set_reference(reference);
        const size_t n = size();
        zsw_batch b = batch();
        std::vector<uint32_t> score(n), rs(n), re(n), qs(n), qe(n);
        std::vector<uint8_t> status(n);
        ctx_.check(zsw_score_ranges_batch(ctx_.raw(), &b, T_, N_, score.data(), rs.data(), re.data(), qs.data(), qe.data(), status.data(), nullptr));
        std::vector<MaybeAligned<ScoreAndRanges>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], ScoreAndRanges{score[i], rs[i], re[i], qs[i], qe[i]}};
        return out;
    }
    // profile.rs:515-519 -> sw_simd_align (striped.rs:449-598); seq_is_query = SeqSrc::Query (alignment/mod.rs:176-190)
    std::vector<MaybeAligned<Alignment>> sw_align(const std::string& seq, bool seq_is_query = false) {
        set_reference(seq);
        zsw_batch b = batch();
        return collect([&](zsw_alignment* aln, uint8_t* st, uint32_t* inc, uint8_t* op, uint64_t cap, uint64_t* total) {
            return zsw_align_batch(ctx_.raw(), &b, T_, N_, seq_is_query, aln, st, inc, op, cap, total, nullptr);
        });
    }
    // profile.rs:546-552 -> sw_align_3pass (three_pass.rs:21-104)
    std::vector<MaybeAligned<Alignment>> sw_align_3pass(const std::string& seq, bool seq_is_query = false) {
        set_reference(seq);
        zsw_batch b = batch();
        return collect([&](zsw_alignment* aln, uint8_t* st, uint32_t* inc, uint8_t* op, uint64_t cap, uint64_t* total) {
            return zsw_align_3pass_batch(ctx_.raw(), &b, T_, N_, seq_is_query, aln, st, inc, op, cap, total, nullptr);
        });
    }

  private:
    zsw_int_type T_;
    int N_;
};

// `reads[i].into_local_profile(&matrix, gap_open, gap_extend)` for a whole batch (nucleotides/mod.rs:262-266):
// LocalProfiles with the i8 -> i16 -> i32 cascade of ProfileSets (profile_set.rs:71-283), lane presets w128/w256/w512.
class LocalProfilesBatch : public ProfileBatchBase {
  public:
    LocalProfilesBatch(GpuContext& ctx, const std::vector<std::string>& reads, const WeightMatrix& matrix, int8_t gap_open,
                       int8_t gap_extend, int preset_bits = 256)
        : ProfileBatchBase(ctx, reads, matrix, gap_open, gap_extend), preset_(preset_bits) {}
    // ProfileSets::sw_score_from_i{8,16,32} (profile_set.rs:71-107)
    std::vector<MaybeAligned<uint32_t>> sw_score_from_i8(const std::string& reference) { return score_from(reference, 8); }
    std::vector<MaybeAligned<uint32_t>> sw_score_from_i16(const std::string& reference) { return score_from(reference, 16); }
    std::vector<MaybeAligned<uint32_t>> sw_score_from_i32(const std::string& reference) { return score_from(reference, 32); }
    // ProfileSets::sw_score_ranges_from_i{8,16,32} (profile_set.rs:313-362)
    std::vector<MaybeAligned<ScoreAndRanges>> sw_score_ranges_from_i8(const std::string& reference) { return ranges_from(reference, 8); }
    std::vector<MaybeAligned<ScoreAndRanges>> sw_score_ranges_from_i16(const std::string& reference) { return ranges_from(reference, 16); }
    std::vector<MaybeAligned<ScoreAndRanges>> sw_score_ranges_from_i32(const std::string& reference) { return ranges_from(reference, 32); }
    // ProfileSets::sw_align_from_i{8,16,32} (profile_set.rs:124-179)
    std::vector<MaybeAligned<Alignment>> sw_align_from_i8(const std::string& seq, bool seq_is_query = false) { return align_from(seq, seq_is_query, 8, false); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i16(const std::string& seq, bool seq_is_query = false) { return align_from(seq, seq_is_query, 16, false); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i32(const std::string& seq, bool seq_is_query = false) { return align_from(seq, seq_is_query, 32, false); }
    // ProfileSets::sw_align_from_i{8,16,32}_3pass (profile_set.rs:212-283)
    std::vector<MaybeAligned<Alignment>> sw_align_from_i8_3pass(const std::string& seq, bool seq_is_query = false) { return align_from(seq, seq_is_query, 8, true); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i16_3pass(const std::string& seq, bool seq_is_query = false) { return align_from(seq, seq_is_query, 16, true); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i32_3pass(const std::string& seq, bool seq_is_query = false) { return align_from(seq, seq_is_query, 32, true); }
    // alignment::sneaky_snake(&reference[ref_start[i]..][..ref_len[i]], read_i, threshold) (sneaky_snake.rs:78-131):
    // true / false per read, Status::Unmapped standing in for `None`.
    std::vector<MaybeAligned<bool>> sneaky_snake(const std::string& reference, const std::vector<uint32_t>& ref_start,
                                                 const std::vector<uint32_t>& ref_len, float threshold) {
        const size_t n = size();
        if (ref_start.size() != n || ref_len.size() != n) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one window per read");
        set_reference(reference);
        zsw_batch b = batch();
        std::vector<uint8_t> pass(n);
        ctx_.check(zsw_sneaky_snake_batch(ctx_.raw(), &b, ref_start.data(), ref_len.data(), threshold, pass.data(), nullptr));
        std::vector<MaybeAligned<bool>> out(n);
        for (size_t i = 0; i < n; ++i) {
            out[i].status = pass[i] == ZSW_FILTER_NONE ? Status::Unmapped : Status::Some;
            out[i].value = pass[i] == ZSW_FILTER_PASS;
        }
        return out;
    }
    // Reads from either strand (zsw_score_strands_batch_from): per read the better of sw_score_from_i{8,16,32} on the read and on
    // its reverse complement (Nucleotides::to_reverse_complement), ties to the forward strand; last_strands() says which it was
    std::vector<MaybeAligned<uint32_t>> sw_score_strands_from_i8(const std::string& reference) { return score_strands_from(reference, 8); }
    std::vector<MaybeAligned<uint32_t>> sw_score_strands_from_i16(const std::string& reference) { return score_strands_from(reference, 16); }
    std::vector<MaybeAligned<uint32_t>> sw_score_strands_from_i32(const std::string& reference) { return score_strands_from(reference, 32); }
    // zsw_align_3pass_strands_batch_from: sw_align_from_i{8,16,32}_3pass of the read or of its reverse complement, whichever scores
    // higher; coordinates are those of the sequence as aligned (a SAM record with flag 16 for strand 1)
    std::vector<MaybeAligned<Alignment>> sw_align_strands_from_i8_3pass(const std::string& seq, bool seq_is_query = false) { return align_strands_from(seq, seq_is_query, 8); }
    std::vector<MaybeAligned<Alignment>> sw_align_strands_from_i16_3pass(const std::string& seq, bool seq_is_query = false) { return align_strands_from(seq, seq_is_query, 16); }
    std::vector<MaybeAligned<Alignment>> sw_align_strands_from_i32_3pass(const std::string& seq, bool seq_is_query = false) { return align_strands_from(seq, seq_is_query, 32); }
    // the strand that answered each read of the last strand-aware call: 0 forward, 1 reverse complement
    const std::vector<uint8_t>& last_strands() const { return strand_; }
    // the reads with every read of strand[i] != 0 replaced by its reverse complement (zsw_orient_batch)
    std::vector<std::string> orient(const std::vector<uint8_t>& strand) {
        if (strand.size() != size()) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one strand per read");
        zsw_batch b = batch();
        std::vector<uint8_t> out(bases_.size());
        ctx_.check(zsw_orient_batch(ctx_.raw(), &b, strand.data(), out.data(), nullptr));
        std::vector<std::string> reads(size());
        for (size_t i = 0; i < size(); ++i) reads[i].assign(out.begin() + offsets_[i], out.begin() + offsets_[i + 1]);
        return reads;
    }
    // Reference panels (zsw_score_panel_batch_from): per read sw_score_from_i{8,16,32} against the member of the context's panel
    // (GpuContext::set_panel) that ranks highest, ties to the lowest member; last_refs() says which it was
    std::vector<MaybeAligned<uint32_t>> sw_score_panel_from_i8() { return score_panel_from(8); }
    std::vector<MaybeAligned<uint32_t>> sw_score_panel_from_i16() { return score_panel_from(16); }
    std::vector<MaybeAligned<uint32_t>> sw_score_panel_from_i32() { return score_panel_from(32); }
    // the member that answered each read of the last panel call
    const std::vector<uint32_t>& last_refs() const { return ref_; }
    // the reads with ref_of[i] == k, in input order (zsw_panel_gather_batch); index: which input read each of them is
    std::vector<std::string> panel_gather(const std::vector<uint32_t>& ref_of, uint32_t k, std::vector<uint32_t>* index = nullptr) {
        if (ref_of.size() != size()) throw GpuError(ZSW_ERR_INVALID_ARGUMENT, "one member per read");
        zsw_batch b = batch();
        std::vector<uint8_t> out(bases_.size() + 1);
        std::vector<uint64_t> off(size() + 1);
        std::vector<uint32_t> idx(size() + 1);
        uint64_t m = 0;
        ctx_.check(zsw_panel_gather_batch(ctx_.raw(), &b, ref_of.data(), k, out.data(), off.data(), idx.data(), &m, nullptr));
        std::vector<std::string> reads(m);
        for (size_t j = 0; j < m; ++j) reads[j].assign(out.begin() + off[j], out.begin() + off[j + 1]);
        idx.resize(m);
        if (index) index->swap(idx);
        return reads;
    }
    // the width that answered each read of the last cascade call (8, 16 or 32)
    const std::vector<uint8_t>& last_tiers() const { return tier_; }

  private:
    std::vector<MaybeAligned<uint32_t>> score_panel_from(int width) {
        const size_t n = size();
        zsw_batch b = batch();
        std::vector<uint32_t> score(n);
        std::vector<uint8_t> status(n);
        tier_.assign(n, 0);
        ref_.assign(n, 0);
        ctx_.check(zsw_score_panel_batch_from(ctx_.raw(), &b, width, preset_, score.data(), status.data(), tier_.data(), ref_.data(), nullptr));
        std::vector<MaybeAligned<uint32_t>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], score[i]};
        return out;
    }
    std::vector<MaybeAligned<Alignment>> align_from(const std::string& seq, bool seq_is_query, int width, bool three_pass) {
        set_reference(seq);
        zsw_batch b = batch();
        tier_.assign(size(), 0);
        return collect([&](zsw_alignment* aln, uint8_t* st, uint32_t* inc, uint8_t* op, uint64_t cap, uint64_t* total) {
            return (three_pass ? zsw_align_3pass_batch_from : zsw_align_batch_from)(ctx_.raw(), &b, width, preset_, seq_is_query, aln, st,
                                                                                   tier_.data(), inc, op, cap, total, nullptr);
        });
    }
    std::vector<MaybeAligned<Alignment>> align_strands_from(const std::string& seq, bool seq_is_query, int width) {
        set_reference(seq);
        zsw_batch b = batch();
        tier_.assign(size(), 0);
        strand_.assign(size(), 0);
        return collect([&](zsw_alignment* aln, uint8_t* st, uint32_t* inc, uint8_t* op, uint64_t cap, uint64_t* total) {
            return zsw_align_3pass_strands_batch_from(ctx_.raw(), &b, width, preset_, seq_is_query, aln, st, tier_.data(), strand_.data(), inc, op, cap, total,
                                                      nullptr);
        });
    }
    std::vector<MaybeAligned<uint32_t>> score_strands_from(const std::string& reference, int width) {
        set_reference(reference);
        const size_t n = size();
        zsw_batch b = batch();
        std::vector<uint32_t> score(n);
        std::vector<uint8_t> status(n);
        tier_.assign(n, 0);
        strand_.assign(n, 0);
        ctx_.check(zsw_score_strands_batch_from(ctx_.raw(), &b, width, preset_, score.data(), status.data(), tier_.data(), strand_.data(), nullptr));
        std::vector<MaybeAligned<uint32_t>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], score[i]};
        return out;
    }
    std::vector<MaybeAligned<ScoreAndRanges>> ranges_from(const std::string& reference, int width) {
        set_reference(reference);
        const size_t n = size();
        zsw_batch b = batch();
        std::vector<uint32_t> score(n), rs(n), re(n), qs(n), qe(n);
        std::vector<uint8_t> status(n);
        tier_.assign(n, 0);
        ctx_.check(zsw_score_ranges_batch_from(ctx_.raw(), &b, width, preset_, score.data(), rs.data(), re.data(), qs.data(), qe.data(),
                                               status.data(), tier_.data(), nullptr));
        std::vector<MaybeAligned<ScoreAndRanges>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], ScoreAndRanges{score[i], rs[i], re[i], qs[i], qe[i]}};
        return out;
    }
    std::vector<MaybeAligned<uint32_t>> score_from(const std::string& reference, int width) {
        set_reference(reference);
        const size_t n = size();
        zsw_batch b = batch();
        std::vector<uint32_t> score(n);
        std::vector<uint8_t> status(n);
        tier_.assign(n, 0);
        ctx_.check(zsw_score_batch_from(ctx_.raw(), &b, width, preset_, score.data(), status.data(), tier_.data(), nullptr));
        std::vector<MaybeAligned<uint32_t>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], score[i]};
        return out;
    }
    int preset_;
    std::vector<uint8_t> tier_, strand_;
    std::vector<uint32_t> ref_;
};

// The other role of the striped functions (sw/mod.rs:63-67; SharedProfiles, profile_set.rs:552-560;
// Nucleotides::into_shared_profile, nucleotides/mod.rs:295-299): ONE profile built from `sequence`, used against every read of a
// batch — the reads are the sequences sw_simd_* walks row by row, so in the results `ref_*` is the read and `query_*` the profile
// sequence unless seq_is_query (SeqSrc::Query(read), alignment/mod.rs:176-190) hands the roles back.
class SharedProfileBase {
  protected:
    SharedProfileBase(GpuContext& ctx, const std::string& sequence, const WeightMatrix& matrix, int8_t gap_open, int8_t gap_extend)
        : ctx_(ctx), seq_len_(sequence.size()) {
        if (sequence.empty()) throw ProfileError(1);  // StripedProfile::new -> ProfileError::EmptySequence (profile.rs:32-44)
        ctx_.check(zsw_set_scoring(ctx_.raw(), matrix.weights.data(), matrix.S, matrix.mapping->index_map.data(), gap_open, gap_extend));
        ctx_.check(zsw_set_profile_sequence(ctx_.raw(), (const uint8_t*)sequence.data(), sequence.size(), ZSW_MEM_HOST));
    }
    // the reads as one host batch (an empty read is an empty `reference` argument: Unmapped, striped.rs:219-221)
    struct HostReads {
        std::vector<uint8_t> bases;
        std::vector<uint64_t> offsets;
        zsw_batch batch() const {
            zsw_batch b;
            b.bases = bases.data();
            b.offsets = offsets.data();
            b.fixed_len = 0;
            b.n_reads = offsets.size() - 1;
            b.mem = ZSW_MEM_HOST;
            b.encoding = ZSW_ENCODING_BYTES;
            return b;
        }
    };
    static HostReads pack(const std::vector<std::string>& reads) {
        HostReads h;
        h.offsets.push_back(0);
        for (auto& r : reads) {
            h.bases.insert(h.bases.end(), r.begin(), r.end());
            h.offsets.push_back(h.bases.size());
        }
        return h;
    }
    template <typename Call>
    std::vector<MaybeAligned<Alignment>> collect(size_t n, Call call) {
        std::vector<zsw_alignment> aln(n);
        std::vector<uint8_t> status(n);
        std::vector<uint32_t> inc(16 * n + 64);
        std::vector<uint8_t> op(inc.size());
        uint64_t total = 0;
        zsw_error e = call(aln.data(), status.data(), inc.data(), op.data(), (uint64_t)inc.size(), &total);
        if (e == ZSW_ERR_INVALID_ARGUMENT && total > inc.size()) {
            inc.resize(total);
            op.resize(total);
            e = call(aln.data(), status.data(), inc.data(), op.data(), (uint64_t)inc.size(), &total);
        }
        ctx_.check(e);
        std::vector<MaybeAligned<Alignment>> out(n);
        for (size_t i = 0; i < n; ++i) {
            out[i].status = (Status)status[i];
            if (status[i] != 0) continue;
            Alignment& a = out[i].value;
            a.score = aln[i].score;
            a.ref_start = aln[i].ref_start;
            a.ref_end = aln[i].ref_end;
            a.query_start = aln[i].query_start;
            a.query_end = aln[i].query_end;
            a.ref_len = aln[i].ref_len;
            a.query_len = aln[i].query_len;
            for (uint32_t k = 0; k < aln[i].n_ciglets; ++k)
                a.states.push_back({inc[aln[i].ciglet_offset + k], op[aln[i].ciglet_offset + k]});
        }
        return out;
    }
    GpuContext& ctx_;
    size_t seq_len_;  // of the profile's sequence

  public:
    // zsw_pileup_batch over the alignments one of this profile's alignment calls returned for `reads` (with the same seq_is_query):
    // the table over the profile's own sequence; results as ProfileBatchBase::pileup
    Pileup pileup(const std::vector<MaybeAligned<Alignment>>& alns, const std::vector<std::string>& reads, bool seq_is_query = true, bool insertions = false,
                  const Pileup* into = nullptr) {
        const HostReads h = pack(reads);
        return ctx_.pileup(h.batch(), ZSW_ANNOTATE_SHARED | (seq_is_query ? 0 : ZSW_ANNOTATE_READ_IS_REF), alns, seq_len_, insertions, into);
    }
    // zsw_annotate_batch over the alignments one of this profile's alignment calls returned for `reads` (with the same seq_is_query);
    // results as ProfileBatchBase::annotate
    Annotation annotate(const std::vector<MaybeAligned<Alignment>>& alns, const std::vector<std::string>& reads, bool seq_is_query = true, bool residues = false,
                        bool verbose = true) {
        const HostReads h = pack(reads);
        return ctx_.annotate(h.batch(), ZSW_ANNOTATE_SHARED | (seq_is_query ? 0 : ZSW_ANNOTATE_READ_IS_REF) | (residues ? ZSW_ANNOTATE_MATCH_RESIDUES : 0), alns, verbose);
    }
};

// `StripedProfile::<T, N, S>::new(sequence, ..)` once; sw_score / sw_score_ends / sw_score_ranges / sw_align against a batch of reads
class SharedStripedProfile : public SharedProfileBase {
  public:
    SharedStripedProfile(GpuContext& ctx, const std::string& sequence, const WeightMatrix& matrix, int8_t gap_open, int8_t gap_extend,
                         zsw_int_type T, int N)
        : SharedProfileBase(ctx, sequence, matrix, gap_open, gap_extend), T_(T), N_(N) {}
    std::vector<MaybeAligned<uint32_t>> sw_score(const std::vector<std::string>& reads) {
        const HostReads h = pack(reads);
        const zsw_batch b = h.batch();
        const size_t n = reads.size();
        std::vector<uint32_t> score(n);
        std::vector<uint8_t> status(n);
        ctx_.check(zsw_score_shared_batch(ctx_.raw(), &b, T_, N_, score.data(), status.data(), nullptr));
        std::vector<MaybeAligned<uint32_t>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], score[i]};
        return out;
    }
    // ref_end: exclusive end in the read, query_end: in the profile sequence (first read position holding the maximum, then the
    // first sequence position)
    std::vector<MaybeAligned<ScoreEnds>> sw_score_ends(const std::vector<std::string>& reads) {
        const HostReads h = pack(reads);
        const zsw_batch b = h.batch();
        const size_t n = reads.size();
        std::vector<uint32_t> score(n), re(n), qe(n);
        std::vector<uint8_t> status(n);
        ctx_.check(zsw_score_ends_shared_batch(ctx_.raw(), &b, T_, N_, score.data(), re.data(), qe.data(), status.data(), nullptr));
        std::vector<MaybeAligned<ScoreEnds>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], ScoreEnds{score[i], re[i], qe[i]}};
        return out;
    }
    std::vector<MaybeAligned<ScoreAndRanges>> sw_score_ranges(const std::vector<std::string>& reads) {
        const HostReads h = pack(reads);
        const zsw_batch b = h.batch();
        const size_t n = reads.size();
        std::vector<uint32_t> score(n), rs(n), re(n), qs(n), qe(n);
        std::vector<uint8_t> status(n);
        ctx_.check(zsw_score_ranges_shared_batch(ctx_.raw(), &b, T_, N_, score.data(), rs.data(), re.data(), qs.data(), qe.data(), status.data(), nullptr));
        std::vector<MaybeAligned<ScoreAndRanges>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], ScoreAndRanges{score[i], rs[i], re[i], qs[i], qe[i]}};
        return out;
    }
    // seq_is_query = true: SeqSrc::Query(read) — the usual call when the profile is the reference
    std::vector<MaybeAligned<Alignment>> sw_align(const std::vector<std::string>& reads, bool seq_is_query = true) {
        const HostReads h = pack(reads);
        const zsw_batch b = h.batch();
        return collect(reads.size(), [&](zsw_alignment* aln, uint8_t* st, uint32_t* inc, uint8_t* op, uint64_t cap, uint64_t* total) {
            return zsw_align_shared_batch(ctx_.raw(), &b, T_, N_, seq_is_query, aln, st, inc, op, cap, total, nullptr);
        });
    }

  private:
    zsw_int_type T_;
    int N_;
};

// `sequence.into_shared_profile(&matrix, gap_open, gap_extend)`: SharedProfiles with the i8 -> i16 -> i32 cascade
class SharedProfilesBatch : public SharedProfileBase {
  public:
    SharedProfilesBatch(GpuContext& ctx, const std::string& sequence, const WeightMatrix& matrix, int8_t gap_open, int8_t gap_extend,
                        int preset_bits = 256)
        : SharedProfileBase(ctx, sequence, matrix, gap_open, gap_extend), preset_(preset_bits) {}
    std::vector<MaybeAligned<uint32_t>> sw_score_from_i8(const std::vector<std::string>& reads) { return score_from(reads, 8); }
    std::vector<MaybeAligned<uint32_t>> sw_score_from_i16(const std::vector<std::string>& reads) { return score_from(reads, 16); }
    std::vector<MaybeAligned<uint32_t>> sw_score_from_i32(const std::vector<std::string>& reads) { return score_from(reads, 32); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i8(const std::vector<std::string>& reads, bool seq_is_query = true) { return align_from(reads, seq_is_query, 8); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i16(const std::vector<std::string>& reads, bool seq_is_query = true) { return align_from(reads, seq_is_query, 16); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i32(const std::vector<std::string>& reads, bool seq_is_query = true) { return align_from(reads, seq_is_query, 32); }
    // ProfileSets::sw_align_from_i*_3pass (profile_set.rs:212-283) of SharedProfiles (:552-560)
    std::vector<MaybeAligned<Alignment>> sw_align_from_i8_3pass(const std::vector<std::string>& reads, bool seq_is_query = true) { return align_from(reads, seq_is_query, 8, true); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i16_3pass(const std::vector<std::string>& reads, bool seq_is_query = true) { return align_from(reads, seq_is_query, 16, true); }
    std::vector<MaybeAligned<Alignment>> sw_align_from_i32_3pass(const std::vector<std::string>& reads, bool seq_is_query = true) { return align_from(reads, seq_is_query, 32, true); }
    const std::vector<uint8_t>& last_tiers() const { return tier_; }

  private:
    std::vector<MaybeAligned<uint32_t>> score_from(const std::vector<std::string>& reads, int width) {
        const HostReads h = pack(reads);
        const zsw_batch b = h.batch();
        const size_t n = reads.size();
        std::vector<uint32_t> score(n);
        std::vector<uint8_t> status(n);
        tier_.assign(n, 0);
        ctx_.check(zsw_score_shared_batch_from(ctx_.raw(), &b, width, preset_, score.data(), status.data(), tier_.data(), nullptr));
        std::vector<MaybeAligned<uint32_t>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {(Status)status[i], score[i]};
        return out;
    }
    std::vector<MaybeAligned<Alignment>> align_from(const std::vector<std::string>& reads, bool seq_is_query, int width, bool three_pass = false) {
        const HostReads h = pack(reads);
        const zsw_batch b = h.batch();
        tier_.assign(reads.size(), 0);
        return collect(reads.size(), [&](zsw_alignment* aln, uint8_t* st, uint32_t* inc, uint8_t* op, uint64_t cap, uint64_t* total) {
            return (three_pass ? zsw_align_3pass_shared_batch_from : zsw_align_shared_batch_from)(ctx_.raw(), &b, width, preset_, seq_is_query, aln, st,
                                                                                                 tier_.data(), inc, op, cap, total, nullptr);
        });
    }
    int preset_;
    std::vector<uint8_t> tier_;
};

}  // namespace zoe
