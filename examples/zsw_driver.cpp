// zsw_driver — C++ host driver over include/zoe_sw.hpp: reads FASTQ records and a one-sequence FASTA/plain reference,
// aligns every read on the GPU (sw_align_from_i8, w256 preset: what `Nucleotides::into_local_profile` users call) and prints
// SAM records with the fields the reference's SamData::from_alignment fills (src/data/records/sam/mod.rs:223-245):
// POS = ref_range.start + 1, CIGAR = states, AS:i = score.
//
//   g++ -O2 -std=c++17 -Iinclude examples/zsw_driver.cpp -o examples/zsw_driver -Lzoe_amd -lzoe_sw_hip -Wl,-rpath,$PWD/zoe_amd
//   ./examples/zsw_driver reference.txt reads.fastq [--score-only | --3pass | --both-strands] [--min-score T] [--nm] [--verbose-cigar] [--device-sam]
//                         [--consensus FILE] [--device-fastq] [--from-sam FILE] [--device-fasta] [--ref-record K] [--fasta-reads] [--panel]
// --both-strands: every read is aligned on whichever strand scores higher (sw_align_strands_from_i8_3pass); a read answered by
// its reverse complement gets flag 16, SEQ reverse complemented and QUAL reversed, and POS / CIGAR are those of that sequence.
// --min-score T (with --3pass or --score-only, the calls ZSW_OPTION_MIN_SCORE covers): a read that scores less than T is written as
// an unmapped record (flag 4; `*` with --score-only), exactly as a read without any alignment is — and costs the GPU next to nothing.
// --nm appends NM:i: (mismatches + inserted + deleted bases) to every mapped record, --verbose-cigar writes the CIGAR with = / X in
// place of M (Alignment::to_verbose_sequence_matching); both come from one zsw_annotate_batch pass over the alignments. Without them
// the output is what it always was.
// --device-sam: the records are formatted on the GPU (zsw_sam_batch) and the body is written with one fwrite; the same bytes as
// without it, under every option above. Without the flag neither the output nor the code path changes.
// --consensus FILE: beside the SAM output, the plurality consensus of the run as a one-record FASTA: the alignments piled up over the
// reference on the GPU (zsw_pileup_batch; under --both-strands from the reads as aligned), per position the most frequent of A C G T N
// (zsw_consensus_from_counts), and the reference's own base where no read covers it.
// --device-fastq: the FASTQ file is read with one fread and parsed on the GPU (zsw_fastq_parse_batch with ZSW_FASTQ_FINAL |
// ZSW_FASTQ_NAME_TO_BLANK) instead of line by line on the host; a malformed record ends the driver with exit status 1 and a message
// naming the code and the record. Everything downstream, and the output, is the same.
// --from-sam FILE: the records come from a SAM file instead of from an alignment call: one fread and one zsw_sam_parse_batch (with
// ZSW_SAMTEXT_FINAL | ZSW_SAMTEXT_QUAL_FORWARD, the loaded reference's name as RNAME and its length as ref_len); the reads argument is
// not opened (pass -). --nm, --verbose-cigar, --device-sam and --consensus work on these records as on aligned ones: run on a file the
// driver wrote, --device-sam writes that file again. A line the reader rejects ends the driver with exit status 1, naming the line.
// --device-fasta: the reference file is read with one fread and parsed on the GPU (zsw_fasta_parse_batch with ZSW_FASTA_FINAL |
// ZSW_FASTA_NAME_TO_BLANK) instead of by the getline loop, which glues the records of a multi-record file together and reports no
// malformed file. Record --ref-record K (default 0) is the reference and its name RNAME. A malformed file ends the driver with exit
// status 1 and a message naming the code and the record. On a one-record file the output is the same as without the flag.
// --fasta-reads: the reads argument is FASTA (contigs, consensus sequences, reads without qualities), parsed on the GPU the same way;
// QUAL is `*`. It does not go with --device-fastq or --from-sam. Without either flag, code path and output are what they were.
// --panel: the reference file is multi-record FASTA, read as under --device-fasta, and every record is a member of a reference panel
// (zsw_set_panel). One zsw_score_panel_batch_from call finds the member each read scores highest against (ties: the first record);
// then per member with reads: zsw_panel_gather_batch, that member as the reference, sw_align_from_i8_3pass on the group. The lines
// come out in input order with the member's name as RNAME, after @HD and one @SQ per record: per read the line that
// `--device-fasta --ref-record K --3pass` writes for the read's best record K (a read unmapped everywhere: record 0's). It goes with
// --device-fastq and --fasta-reads only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

#include "zoe_sw.hpp"

static std::string read_reference(const std::string& path, std::string* name) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::string line, seq;
    *name = "ref";
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() && line[0] == '>') {
            std::istringstream ss(line.substr(1));
            ss >> *name;
        } else {
            seq += line;
        }
    }
    return seq;
}

static std::string read_whole(const std::string& path) {
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::string text(size > 0 ? (size_t)size : 0, '\0');
    const size_t got = text.empty() ? 0 : std::fread(&text[0], 1, text.size(), f);
    std::fclose(f);
    if (got != text.size()) throw std::runtime_error("cannot read " + path);
    return text;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::cerr << "usage: zsw_driver reference.(fa|txt) reads.fastq [--score-only | --3pass | --both-strands] [--min-score T] [--nm] [--verbose-cigar] [--device-sam] [--consensus FILE] [--device-fastq] [--from-sam FILE] [--device-fasta] [--ref-record K] [--fasta-reads] [--panel]\n";
        return 2;
    }
    bool score_only = false, three_pass = false, both_strands = false, nm = false, verbose_cigar = false, device_sam = false, device_fastq = false, device_fasta = false, fasta_reads = false;
    bool panel = false;
    long long min_score = 0, ref_record = 0;
    std::string consensus_path, from_sam;
    for (int k = 3; k < argc; ++k) {
        if (!std::strcmp(argv[k], "--score-only")) score_only = true;
        else if (!std::strcmp(argv[k], "--3pass")) three_pass = true;  // sw_align_from_i8_3pass instead of sw_align_from_i8
        else if (!std::strcmp(argv[k], "--both-strands")) both_strands = true;  // sw_align_strands_from_i8_3pass
        else if (!std::strcmp(argv[k], "--min-score") && k + 1 < argc) min_score = std::atoll(argv[++k]);
        else if (!std::strcmp(argv[k], "--nm")) nm = true;
        else if (!std::strcmp(argv[k], "--verbose-cigar")) verbose_cigar = true;
        else if (!std::strcmp(argv[k], "--device-sam")) device_sam = true;
        else if (!std::strcmp(argv[k], "--device-fastq")) device_fastq = true;
        else if (!std::strcmp(argv[k], "--device-fasta")) device_fasta = true;
        else if (!std::strcmp(argv[k], "--fasta-reads")) fasta_reads = true;
        else if (!std::strcmp(argv[k], "--ref-record") && k + 1 < argc) ref_record = std::atoll(argv[++k]);
        else if (!std::strcmp(argv[k], "--consensus") && k + 1 < argc) consensus_path = argv[++k];
        else if (!std::strcmp(argv[k], "--from-sam") && k + 1 < argc) from_sam = argv[++k];
        else if (!std::strcmp(argv[k], "--panel")) panel = true;
        else {
            std::cerr << "zsw_driver: unknown argument " << argv[k] << '\n';
            return 2;
        }
    }
    if (min_score < 0 || min_score > 0x7fffffffll || (min_score > 0 && !(score_only || three_pass))) {
        std::cerr << "zsw_driver: --min-score takes a value in 1 .. 2^31 - 1 and goes with --3pass or --score-only\n";
        return 2;
    }
    if (score_only && !consensus_path.empty()) {
        std::cerr << "zsw_driver: --consensus needs alignments; it does not go with --score-only\n";
        return 2;
    }
    if (!from_sam.empty() && (score_only || three_pass || both_strands || min_score > 0 || device_fastq)) {
        std::cerr << "zsw_driver: --from-sam takes its records from the file; it goes with --nm, --verbose-cigar, --device-sam and --consensus only\n";
        return 2;
    }
    if (fasta_reads && (device_fastq || !from_sam.empty())) {
        std::cerr << "zsw_driver: --fasta-reads does not go with --device-fastq or --from-sam\n";
        return 2;
    }
    if (ref_record < 0 || (ref_record > 0 && !device_fasta)) {
        std::cerr << "zsw_driver: --ref-record takes an index from 0 and goes with --device-fasta\n";
        return 2;
    }
    if (panel && (both_strands || !from_sam.empty() || !consensus_path.empty())) {
        std::cerr << "zsw_driver: --panel does not go with --both-strands, --from-sam or --consensus\n";
        return 2;
    }
    if (panel && (score_only || min_score > 0 || nm || verbose_cigar || device_sam || ref_record > 0)) {
        std::cerr << "zsw_driver: --panel writes the plain SAM lines of the 3-pass call; it does not go with --score-only, --min-score, --nm, --verbose-cigar, "
                     "--device-sam or --ref-record\n";
        return 2;
    }
    try {
        std::string ref_name;
        std::unique_ptr<zoe::GpuContext> ctx_holder;
        // a FASTA file with one fread, its records from zsw_fasta_parse_batch; a malformed file is an error that names code and record
        const auto parse_fasta_file = [&](const char* path) {
            if (!ctx_holder) ctx_holder.reset(new zoe::GpuContext(0));
            zoe::FastaRecords fa = ctx_holder->parse_fasta(read_whole(path), true, true);
            if (fa.error())
                throw std::runtime_error(std::string("malformed FASTA ") + path + ": code " + std::to_string(fa.error()) + " at record " +
                                         std::to_string(fa.report[ZSW_FASTA_INFO_ERROR_RECORD]) + " (byte " + std::to_string(fa.report[ZSW_FASTA_INFO_ERROR_OFFSET]) + "): " +
                                         zoe::FastaRecords::error_text(fa.error()));
            return fa;
        };
        std::string reference;
        zoe::FastaRecords panel_fa;  // --panel: every record of the reference file is a member
        if (panel) {
            panel_fa = parse_fasta_file(argv[1]);
            if (panel_fa.sequences.empty() || panel_fa.sequences.size() > ZSW_PANEL_MAX_REFS)
                throw std::runtime_error("--panel: the file has " + std::to_string(panel_fa.sequences.size()) + " records; a panel holds 1 to " +
                                         std::to_string(ZSW_PANEL_MAX_REFS));
        } else if (device_fasta) {
            zoe::FastaRecords fa = parse_fasta_file(argv[1]);
            if ((size_t)ref_record >= fa.sequences.size())
                throw std::runtime_error("--ref-record " + std::to_string(ref_record) + ": the file has " + std::to_string(fa.sequences.size()) + " records");
            reference = std::move(fa.sequences[(size_t)ref_record]);
            ref_name = std::move(fa.names[(size_t)ref_record]);
        } else {
            reference = read_reference(argv[1], &ref_name);
        }
        std::vector<std::string> names, reads, quals;
        std::vector<zoe::MaybeAligned<zoe::Alignment>> sam_alns;
        std::vector<uint8_t> sam_strands;
        if (!from_sam.empty()) {  // the whole file with one fread, records and reads from zsw_sam_parse_batch
            const std::string text = read_whole(from_sam);
            ctx_holder.reset(new zoe::GpuContext(0));
            zoe::SamRecords sam = ctx_holder->parse_sam(text, true, true, ref_name, (uint32_t)reference.size());
            if (sam.error())
                throw std::runtime_error("malformed SAM: line " + std::to_string(sam.report[ZSW_SAMTEXT_INFO_ERROR_LINE] + 1) + " (byte " +
                                         std::to_string(sam.report[ZSW_SAMTEXT_INFO_ERROR_OFFSET]) + "): " + zoe::SamRecords::error_text(sam.error()) + " (code " +
                                         std::to_string(sam.error()) + ")");
            names = std::move(sam.names);
            quals = std::move(sam.quals);
            sam_alns = std::move(sam.alns);
            sam_strands = std::move(sam.strands);
            // SEQ is the read as aligned; the profile classes take the reads as sequenced and orient them by strand
            const zoe::WeightMatrix w = zoe::WeightMatrix::new_dna_matrix(2, -5, 'N');
            reads = sam.reads.empty() ? sam.reads : zoe::LocalProfilesBatch(*ctx_holder, sam.reads, w, -10, -1).orient(sam_strands);
        } else if (device_fastq) {  // the whole file with one fread, the records from zsw_fastq_parse_batch
            const std::string text = read_whole(argv[2]);
            ctx_holder.reset(new zoe::GpuContext(0));
            zoe::FastqRecords fastq = ctx_holder->parse_fastq(text, true, true);
            if (fastq.error())
                throw std::runtime_error("malformed FASTQ: code " + std::to_string(fastq.error()) + " at record " + std::to_string(fastq.report[ZSW_FASTQ_INFO_ERROR_RECORD]) +
                                         " (byte " + std::to_string(fastq.report[ZSW_FASTQ_INFO_ERROR_OFFSET]) + ")");
            names = std::move(fastq.names);
            reads = std::move(fastq.reads);
            quals = std::move(fastq.quals);
        } else if (fasta_reads) {
            zoe::FastaRecords fa = parse_fasta_file(argv[2]);
            names = std::move(fa.names);
            reads = std::move(fa.sequences);
            quals.assign(reads.size(), "*");  // there are no qualities
        } else {
            std::ifstream fq(argv[2]);
            if (!fq) throw std::runtime_error(std::string("cannot open ") + argv[2]);
            std::string h, s, p, q;
            while (std::getline(fq, h) && std::getline(fq, s) && std::getline(fq, p) && std::getline(fq, q)) {
                if (h.empty() || h[0] != '@') throw std::runtime_error("malformed FASTQ header: " + h);
                names.push_back(h.substr(1, h.find_first_of(" \t") == std::string::npos ? std::string::npos : h.find_first_of(" \t") - 1));
                reads.push_back(s);
                quals.push_back(q);
            }
        }
        if (!ctx_holder) ctx_holder.reset(new zoe::GpuContext(0));
        zoe::GpuContext& ctx = *ctx_holder;
        if (min_score > 0) ctx.set_min_score((uint32_t)min_score);
        const zoe::WeightMatrix weights = zoe::WeightMatrix::new_dna_matrix(2, -5, 'N');
        zoe::LocalProfilesBatch profiles(ctx, reads, weights, -10, -1);
        if (panel) {  // the member each read belongs to from one panel call, then per member the 3-pass call on its gathered group
            const std::vector<std::string>& members = panel_fa.sequences;
            ctx.set_panel(members);
            profiles.sw_score_panel_from_i8();
            const std::vector<uint32_t> refs = profiles.last_refs();
            std::vector<std::string> lines(reads.size());
            for (uint32_t k = 0; k < members.size(); ++k) {
                std::vector<uint32_t> index;
                const std::vector<std::string> group = profiles.panel_gather(refs, k, &index);
                if (group.empty()) continue;
                zoe::LocalProfilesBatch group_profiles(ctx, group, weights, -10, -1);
                const auto alns = group_profiles.sw_align_from_i8_3pass(members[k]);
                for (size_t j = 0; j < group.size(); ++j) {
                    const size_t i = index[j];
                    std::ostringstream line;
                    if (alns[j].is_some()) {
                        const zoe::Alignment& a = alns[j].value;
                        line << names[i] << "\t0\t" << panel_fa.names[k] << '\t' << a.ref_start + 1 << "\t255\t" << a.cigar() << "\t*\t0\t0\t" << reads[i] << '\t' << quals[i]
                             << "\tAS:i:" << a.score << '\n';
                    } else {
                        line << names[i] << "\t4\t*\t0\t0\t*\t*\t0\t0\t" << reads[i] << '\t' << quals[i] << '\n';
                    }
                    lines[i] = line.str();
                }
            }
            std::cout << "@HD\tVN:1.6\n";
            for (size_t k = 0; k < members.size(); ++k) std::cout << "@SQ\tSN:" << panel_fa.names[k] << "\tLN:" << members[k].size() << '\n';
            for (const std::string& line : lines) std::cout << line;
            return 0;
        }
        if (score_only) {
            auto scores = profiles.sw_score_from_i8(reference);
            for (size_t i = 0; i < reads.size(); ++i)
                std::cout << names[i] << '\t' << (scores[i].is_some() ? std::to_string(scores[i].value) : std::string("*")) << '\n';
            return 0;
        }
        auto alns = !from_sam.empty() ? std::move(sam_alns)
                    : both_strands  ? profiles.sw_align_strands_from_i8_3pass(reference)
                    : three_pass    ? profiles.sw_align_from_i8_3pass(reference)
                                    : profiles.sw_align_from_i8(reference);
        // which strand each alignment is of: from a strand-aware call, or FLAG & 16 of the file's lines
        const std::vector<uint8_t>* strands = !from_sam.empty() ? &sam_strands : both_strands ? &profiles.last_strands() : nullptr;
        if (!consensus_path.empty()) {
            const zoe::Pileup pile = profiles.pileup(alns, reference, false, false, strands);
            std::ofstream fa(consensus_path);
            if (!fa) throw std::runtime_error("cannot write " + consensus_path);
            fa << '>' << ref_name << "_consensus\n" << ctx.plurality_acgtn(pile.counts, &reference) << '\n';
        }
        zoe::Annotation ann;  // NM and = / X CIGARs: one pass over the alignments, against the reads as aligned
        if (nm || verbose_cigar) ann = profiles.annotate(alns, reference, false, false, verbose_cigar, strands);
        if (device_sam) {  // the body from zsw_sam_batch: SEQ oriented, QUAL reversed and the decimals written on the device
            std::cout << "@HD\tVN:1.6\n@SQ\tSN:" << ref_name << "\tLN:" << reference.size() << '\n' << std::flush;
            const std::string text = profiles.sam_text(verbose_cigar ? ann.verbose : alns, names, fasta_reads ? std::vector<std::string>() : quals, ref_name, 255, strands, nm ? &ann : nullptr);
            std::fwrite(text.data(), 1, text.size(), stdout);
            return 0;
        }
        std::vector<uint8_t> strand(reads.size(), 0);
        if (strands) {  // SEQ and QUAL as aligned: the reverse complement of a read answered on the reverse strand, its qualities reversed
            strand = *strands;
            reads = profiles.orient(strand);
            for (size_t i = 0; i < reads.size(); ++i)
                if (strand[i]) std::reverse(quals[i].begin(), quals[i].end());
        }
        std::cout << "@HD\tVN:1.6\n@SQ\tSN:" << ref_name << "\tLN:" << reference.size() << '\n';
        for (size_t i = 0; i < reads.size(); ++i) {
            if (alns[i].is_some()) {
                const zoe::Alignment& a = alns[i].value;
                std::cout << names[i] << '\t' << (strand[i] ? 16 : 0) << '\t' << ref_name << '\t' << a.ref_start + 1 << "\t255\t"
                          << (verbose_cigar ? ann.verbose[i].value.cigar() : a.cigar()) << "\t*\t0\t0\t" << reads[i] << '\t' << quals[i] << "\tAS:i:" << a.score;
                if (nm) std::cout << "\tNM:i:" << ann.nm(i);
                std::cout << '\n';
            } else {
                std::cout << names[i] << "\t4\t*\t0\t0\t*\t*\t0\t0\t" << reads[i] << '\t' << quals[i] << '\n';
            }
        }
    } catch (const std::exception& e) {
        std::cerr << "zsw_driver: " << e.what() << '\n';
        return 1;
    }
    return 0;
}
