"""ctypes binding of libzoe_sw_hip.so (the C ABI declared in include/zoe_sw.h).

There is no CPU fallback: if the HIP library is missing or no gfx950 device is usable, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzoe_sw_hip.so")

ZSW_OK = 0
ERROR_NAMES = {
    0: "ZSW_OK",
    1: "ProfileError::EmptySequence",
    2: "ProfileError::GapOpenOutOfRange",
    3: "ProfileError::GapExtendOutOfRange",
    4: "ProfileError::BadGapWeights",
    -1: "ZSW_ERR_INVALID_ARGUMENT",
    -2: "ZSW_ERR_HIP",
    -3: "ZSW_ERR_NO_DEVICE",
    -4: "ZSW_ERR_UNSUPPORTED",
    -5: "ZSW_ERR_NOT_CONFIGURED",
}
MEM_HOST, MEM_DEVICE = 0, 1
# zsw_debug_flag (kernel-selection overrides for the parity tests; results never depend on them)
DEBUG_SCORE_V1, DEBUG_NO_TILES, DEBUG_NO_W32, DEBUG_NO_WIDE, DEBUG_NO_SIDE_STREAMS, DEBUG_NO_PIPELINE, DEBUG_ALIGN_NO_PACKED = 1, 2, 4, 8, 16, 32, 64
DEBUG_SCORE_PRUNE, DEBUG_SCORE_PRUNE_ANY_SIZE, DEBUG_PRUNE_STRIP, DEBUG_ALIGN_LONG_WARMUP, DEBUG_SEED_NO_BAND, DEBUG_SEED_WIDE_BAND = 128, 256, 512, 1024, 2048, 4096
DEBUG_NO_ROW_CHUNKS = 8192
DEBUG_RANGES_EXACT_REVERSE = 16384
DEBUG_ALIGN_NO_CERTIFICATE = 32768
DEBUG_SEED_STRIP_FIRST_TIER = 65536
DEBUG_SEED_DIAG_LANE_EVENTS = 131072
DEBUG_SEED_NO_COSCHEDULE = 262144
DEBUG_SEED_PLAIN_KERNEL = 524288
DEBUG_SEED_DIAG_MASKED = 1048576
DEBUG_SEED_NO_SLICES = 2097152
DEBUG_SEED_TINY_SLICES = 4194304
# zsw_launch_kind: the first entry of a zsw_debug_score_launches record
(LAUNCH_V1_FAST, LAUNCH_V1_BIASED, LAUNCH_V2, LAUNCH_WIDE, LAUNCH_V1_FAST_REV, LAUNCH_V1_BIASED_REV, LAUNCH_WIDE_REV, LAUNCH_TILE_V2, LAUNCH_TILE_WIDE,
 LAUNCH_TILE_W32, LAUNCH_EXACT32, LAUNCH_EXACT32_WORKLIST, LAUNCH_SEED_WINDOW, LAUNCH_SEED_BAND, LAUNCH_PRUNED, LAUNCH_ROW_CHUNKS) = range(16)
OPTION_EXACT_PRUNING = 1
OPTION_MIN_SCORE = 2
INT_TYPES = {"i8": 0, "i16": 1, "i32": 2, "u8": 3, "u16": 4, "u32": 5}

# every symbol include/zoe_sw.h declares (tests/test_capi_symbols.py checks the two lists agree)
SYMBOLS = [
    "zsw_pack4_host", "zsw_create", "zsw_destroy", "zsw_last_error_string", "zsw_device_count", "zsw_set_scoring", "zsw_set_reference",
    "zsw_score_batch", "zsw_score_batch_from", "zsw_score_ends_batch", "zsw_score_ranges_batch", "zsw_score_ranges_batch_from", "zsw_align_batch", "zsw_align_batch_from", "zsw_align_3pass_batch", "zsw_align_3pass_batch_from", "zsw_sneaky_snake_batch",
    "zsw_set_profile_sequence", "zsw_score_shared_batch", "zsw_score_shared_batch_from", "zsw_score_ends_shared_batch", "zsw_score_ranges_shared_batch",
    "zsw_score_ranges_shared_batch_from", "zsw_align_shared_batch", "zsw_align_shared_batch_from", "zsw_align_3pass_shared_batch", "zsw_align_3pass_shared_batch_from",
    "zsw_synth_reads", "zsw_synth_reads_ragged", "zsw_synth_length", "zsw_synth_reference_host", "zsw_synth_reads_host",
    "zsw_synth_reads_ragged_host", "zsw_selftest", "zsw_timing_enable", "zsw_timing_read", "zsw_timing_read_window", "zsw_debug_set", "zsw_debug_band_records", "zsw_debug_cert_records", "zsw_debug_threepass_records", "zsw_prune_rescored", "zsw_set_option",
    "zsw_group_create", "zsw_group_destroy", "zsw_group_size", "zsw_group_context", "zsw_group_last_error_string", "zsw_group_set_scoring",
    "zsw_group_set_reference", "zsw_group_score_batch_from", "zsw_group_score_batch_from_device", "zsw_group_align_batch_from",
    "zsw_group_align_3pass_batch_from",
    "zsw_set_complement", "zsw_score_strands_batch_from", "zsw_orient_batch", "zsw_align_3pass_strands_batch_from", "zsw_strand_counts", "zsw_debug_strand_records", "zsw_debug_score_launches",
    "zsw_min_score_counts", "zsw_annotate_batch", "zsw_sam_batch", "zsw_pileup_batch", "zsw_consensus_from_counts", "zsw_fastq_parse_batch",
    "zsw_sam_parse_batch", "zsw_fasta_parse_batch",
    "zsw_set_panel", "zsw_score_panel_batch_from", "zsw_panel_gather_batch", "zsw_panel_counts", "zsw_debug_panel_records",
]
PANEL_MAX_REFS = 64


class ZswBatch(C.Structure):
    _fields_ = [
        ("bases", C.c_void_p),
        ("offsets", C.c_void_p),
        ("fixed_len", C.c_uint32),
        ("n_reads", C.c_uint64),
        ("mem", C.c_int),
        ("encoding", C.c_int),
    ]


class ZswAlignment(C.Structure):
    _fields_ = [
        ("score", C.c_uint32),
        ("ref_start", C.c_uint32),
        ("ref_end", C.c_uint32),
        ("query_start", C.c_uint32),
        ("query_end", C.c_uint32),
        ("ref_len", C.c_uint32),
        ("query_len", C.c_uint32),
        ("n_ciglets", C.c_uint32),
        ("ciglet_offset", C.c_uint64),
    ]


class ZswAlignmentStats(C.Structure):
    _fields_ = [
        ("matches", C.c_uint32),
        ("mismatches", C.c_uint32),
        ("ins_bases", C.c_uint32),
        ("del_bases", C.c_uint32),
        ("ins_runs", C.c_uint32),
        ("del_runs", C.c_uint32),
        ("path_score", C.c_int32),
        ("path_status", C.c_uint32),
    ]


# zsw_path_status and the flags of zsw_annotate_batch
(PATH_OK, PATH_REFERENCE_ENDED, PATH_QUERY_ENDED, PATH_FULL_QUERY_NOT_USED, PATH_FULL_REFERENCE_NOT_USED, PATH_INVALID_CIGAR_OP, PATH_NEGATIVE_SCORE,
 PATH_NO_ALIGNMENT, PATH_BAD_RECORD) = range(9)
ANNOTATE_READ_IS_REF, ANNOTATE_SHARED, ANNOTATE_MATCH_RESIDUES = 1, 2, 4


class ZswSamFields(C.Structure):
    """zsw_sam_fields: what a SAM line holds beside the record; every array lives where the batch does, but rname (host)"""
    _fields_ = [
        ("qnames", C.c_void_p),
        ("qname_offsets", C.c_void_p),
        ("quals", C.c_void_p),
        ("strand", C.c_void_p),
        ("stats", C.c_void_p),
        ("rname", C.c_char_p),
        ("rname_len", C.c_uint32),
        ("mapq", C.c_uint32),
    ]


SAM_OMIT_SEQ = 1

# zsw_pileup_batch / zsw_consensus_from_counts: the flag beside the ANNOTATE_* role bits, the bins of a zsw_site_counts
PILEUP_CLEAR = 8
CONSENSUS_KEEP_UNCOVERED = 1
PILEUP_BINS = ("A", "C", "G", "T", "N", "-", "other", "invalid")

# zsw_fastq_parse_batch: flags, the codes of a record's first failing check, the words of the report
FASTQ_FINAL, FASTQ_NAME_TO_BLANK = 1, 2
(FASTQ_MISSING_AT, FASTQ_MISSING_HEADER, FASTQ_INVALID_UTF8, FASTQ_MISSING_SEQUENCE, FASTQ_MISSING_PLUS, FASTQ_MISSING_QUALITY, FASTQ_LENGTH_MISMATCH,
 FASTQ_INVALID_QUALITY) = range(1, 9)
(FASTQ_INFO_RECORDS, FASTQ_INFO_BASES, FASTQ_INFO_NAME_BYTES, FASTQ_INFO_CONSUMED, FASTQ_INFO_ERROR, FASTQ_INFO_ERROR_RECORD, FASTQ_INFO_ERROR_OFFSET,
 FASTQ_INFO_MIN_LEN, FASTQ_INFO_MAX_LEN, FASTQ_INFO_WORDS) = range(10)

# zsw_fasta_parse_batch: flags, the codes of the first failing check, the words of the report (those of zsw_fastq_parse_batch)
FASTA_FINAL, FASTA_NAME_TO_BLANK, FASTA_CONTINUED = 1, 2, 4
(FASTA_NO_DATA, FASTA_MISSING_GT, FASTA_MISSING_HEADER, FASTA_GT_IN_HEADER, FASTA_MISSING_SEQUENCE, FASTA_GT_IN_SEQUENCE) = range(1, 7)
(FASTA_INFO_RECORDS, FASTA_INFO_BASES, FASTA_INFO_NAME_BYTES, FASTA_INFO_CONSUMED, FASTA_INFO_ERROR, FASTA_INFO_ERROR_RECORD, FASTA_INFO_ERROR_OFFSET,
 FASTA_INFO_MIN_LEN, FASTA_INFO_MAX_LEN, FASTA_INFO_WORDS) = range(10)

# zsw_sam_parse_batch: flags, the reader's codes (SAMTEXT_*), the conversion's codes and bits (SAMREC_*), the words of the report
SAMTEXT_FINAL, SAMTEXT_QUAL_FORWARD = 1, 2
(SAMTEXT_INVALID_UTF8, SAMTEXT_TOO_FEW_FIELDS, SAMTEXT_INVALID_FLAG, SAMTEXT_INVALID_POS, SAMTEXT_INVALID_MAPQ, SAMTEXT_INVALID_QUALITY) = range(1, 7)
(SAMREC_SEQ_MISSING, SAMREC_CIGAR_INVALID_OP, SAMREC_CIGAR_MISSING_INC, SAMREC_CIGAR_INC_ZERO, SAMREC_CIGAR_INC_OVERFLOW, SAMREC_CIGAR_MISSING_OP,
 SAMREC_CIGAR_MERGE_OVERFLOW, SAMREC_POS_ZERO, SAMREC_CLIPS_EXCEED_SEQ, SAMREC_TOO_LARGE) = range(1, 11)
SAMREC_BIT_NO_SCORE, SAMREC_BIT_OTHER_RNAME, SAMREC_BIT_SEQ_MISSING, SAMREC_BIT_QUAL_MISSING, SAMREC_BIT_QUAL_LENGTH = 1, 2, 4, 8, 16
(SAMTEXT_INFO_RECORDS, SAMTEXT_INFO_HEADERS, SAMTEXT_INFO_BASES, SAMTEXT_INFO_NAME_BYTES, SAMTEXT_INFO_CIGLETS, SAMTEXT_INFO_CONSUMED, SAMTEXT_INFO_ERROR,
 SAMTEXT_INFO_ERROR_LINE, SAMTEXT_INFO_ERROR_OFFSET, SAMTEXT_INFO_MAPPED, SAMTEXT_INFO_CODED, SAMTEXT_INFO_MIN_LEN, SAMTEXT_INFO_MAX_LEN,
 SAMTEXT_INFO_WORDS) = range(14)


class ZswSamParsed(C.Structure):
    """zsw_sam_parsed: what a delivered SAM line holds beside its zsw_alignment"""
    _fields_ = [("pos", C.c_uint64), ("line", C.c_uint64), ("flag", C.c_uint16), ("mapq", C.c_uint8), ("code", C.c_uint8), ("bits", C.c_uint32)]


class ZswSamParseOut(C.Structure):
    """zsw_sam_parse_out: the output arrays of zsw_sam_parse_batch and their capacities, in entries"""
    _fields_ = [
        ("bases", C.c_void_p), ("quals", C.c_void_p), ("base_cap", C.c_uint64), ("offsets", C.c_void_p),
        ("qnames", C.c_void_p), ("name_cap", C.c_uint64), ("qname_offsets", C.c_void_p),
        ("aln", C.c_void_p), ("status", C.c_void_p),
        ("inc", C.c_void_p), ("op", C.c_void_p), ("ciglet_cap", C.c_uint64),
        ("strand", C.c_void_p), ("parsed", C.c_void_p), ("record_cap", C.c_uint64),
    ]


class ZswError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        name = ERROR_NAMES.get(code, str(code))
        super().__init__(f"{name}{': ' + detail if detail else ''}")


_lib = None


def load() -> C.CDLL:
    """Loads the HIP library; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZswError(-3, f"{LIB_PATH} not built: run `python -m zoe_amd.build` (hipcc, gfx950)")
    # PyTorch owns device memory and streams here and bundles its own libamdhip64 (SONAME libamdhip64.so.7).
    # It must be loaded first so that this library binds to the SAME HIP runtime instance; the other order
    # puts two runtimes in one process and torch's device pointers would mean nothing to ours.
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    lib.zsw_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.zsw_destroy.argtypes = [vp]
    lib.zsw_destroy.restype = None
    lib.zsw_last_error_string.argtypes = [vp]
    lib.zsw_last_error_string.restype = C.c_char_p
    lib.zsw_set_scoring.argtypes = [vp, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.zsw_set_reference.argtypes = [vp, C.c_void_p, C.c_size_t, C.c_int]
    lib.zsw_score_batch.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, u32p, u8p, vp]
    lib.zsw_score_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, u32p, u8p, u8p, vp]
    lib.zsw_score_ends_batch.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, u32p, u32p, u32p, u8p, vp]
    lib.zsw_score_ranges_batch.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, u32p, u32p, u32p, u32p, u32p, u8p, vp]
    lib.zsw_score_ranges_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, u32p, u32p, u32p, u32p, u32p, u8p, u8p, vp]
    lib.zsw_align_batch.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, C.c_int, vp, u8p, u32p, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    lib.zsw_align_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, C.c_int, vp, u8p, u8p, u32p, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    lib.zsw_align_3pass_batch.argtypes = lib.zsw_align_batch.argtypes
    lib.zsw_align_3pass_batch_from.argtypes = lib.zsw_align_batch_from.argtypes
    lib.zsw_set_profile_sequence.argtypes = [vp, C.c_void_p, C.c_size_t, C.c_int]
    lib.zsw_score_shared_batch.argtypes = lib.zsw_score_batch.argtypes
    lib.zsw_score_shared_batch_from.argtypes = lib.zsw_score_batch_from.argtypes
    lib.zsw_score_ends_shared_batch.argtypes = lib.zsw_score_ends_batch.argtypes
    lib.zsw_score_ranges_shared_batch.argtypes = lib.zsw_score_ranges_batch.argtypes
    lib.zsw_score_ranges_shared_batch_from.argtypes = lib.zsw_score_ranges_batch_from.argtypes
    lib.zsw_align_shared_batch.argtypes = lib.zsw_align_batch.argtypes
    lib.zsw_align_shared_batch_from.argtypes = lib.zsw_align_batch_from.argtypes
    lib.zsw_align_3pass_shared_batch.argtypes = lib.zsw_align_shared_batch.argtypes
    lib.zsw_align_3pass_shared_batch_from.argtypes = lib.zsw_align_batch_from.argtypes
    lib.zsw_sneaky_snake_batch.argtypes = [vp, C.POINTER(ZswBatch), u32p, u32p, C.c_float, u8p, vp]
    lib.zsw_synth_reads.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp]
    lib.zsw_synth_reads_ragged.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, u64p, vp, vp]
    lib.zsw_synth_length.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.zsw_synth_length.restype = C.c_uint32
    lib.zsw_synth_reference_host.argtypes = [C.c_uint64, C.c_uint64, vp]
    lib.zsw_synth_reference_host.restype = None
    lib.zsw_synth_reads_host.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp]
    lib.zsw_synth_reads_host.restype = None
    lib.zsw_synth_reads_ragged_host.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, u64p, vp, C.c_uint32, vp]
    lib.zsw_synth_reads_ragged_host.restype = None
    lib.zsw_selftest.argtypes = [vp]
    lib.zsw_timing_enable.argtypes = [vp, C.c_int]
    lib.zsw_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.zsw_timing_read_window.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.zsw_debug_set.argtypes = [vp, C.c_uint32]
    lib.zsw_debug_band_records.argtypes = [vp, vp]
    lib.zsw_debug_cert_records.argtypes = [vp, vp]
    lib.zsw_debug_threepass_records.argtypes = [vp, vp]
    lib.zsw_pack4_host.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp]
    lib.zsw_prune_rescored.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.zsw_set_option.argtypes = [vp, C.c_int, C.c_int64]
    lib.zsw_group_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    lib.zsw_group_destroy.argtypes = [vp]
    lib.zsw_group_destroy.restype = None
    lib.zsw_group_size.argtypes = [vp]
    lib.zsw_group_context.argtypes = [vp, C.c_int]
    lib.zsw_group_context.restype = vp
    lib.zsw_group_last_error_string.argtypes = [vp]
    lib.zsw_group_last_error_string.restype = C.c_char_p
    lib.zsw_group_set_scoring.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int]
    lib.zsw_group_set_reference.argtypes = [vp, vp, C.c_size_t]
    lib.zsw_group_score_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, vp, vp, vp]
    lib.zsw_group_score_batch_from_device.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    lib.zsw_group_align_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.zsw_group_align_3pass_batch_from.argtypes = lib.zsw_group_align_batch_from.argtypes
    lib.zsw_set_complement.argtypes = [vp, vp]
    lib.zsw_score_strands_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, u32p, u8p, u8p, u8p, vp]
    lib.zsw_orient_batch.argtypes = [vp, C.POINTER(ZswBatch), u8p, u8p, vp]
    lib.zsw_align_3pass_strands_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, C.c_int, vp, u8p, u8p, u8p, u32p, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    lib.zsw_strand_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.zsw_debug_strand_records.argtypes = [vp, vp]
    lib.zsw_debug_score_launches.argtypes = [vp, u32p, C.c_uint32, u32p]
    lib.zsw_min_score_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.zsw_annotate_batch.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, vp, u8p, u32p, u8p, C.c_uint64, vp, vp, u32p, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    lib.zsw_sam_batch.argtypes = [vp, C.POINTER(ZswBatch), C.POINTER(ZswSamFields), C.c_int, vp, u8p, u32p, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64),
                                  u64p, C.POINTER(C.c_uint64), vp]
    lib.zsw_pileup_batch.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, vp, u8p, u32p, u8p, C.c_uint64, vp, vp, C.POINTER(C.c_uint64), vp]
    lib.zsw_consensus_from_counts.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, u8p, u8p, vp]
    lib.zsw_fastq_parse_batch.argtypes = [vp, u8p, C.c_uint64, C.c_int, C.c_int, u8p, u8p, C.c_uint64, u64p, u8p, C.c_uint64, u64p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    lib.zsw_sam_parse_batch.argtypes = [vp, u8p, C.c_uint64, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(ZswSamParseOut), C.POINTER(C.c_uint64), vp]
    lib.zsw_fasta_parse_batch.argtypes = [vp, u8p, C.c_uint64, C.c_int, C.c_int, u8p, C.c_uint64, u64p, u8p, C.c_uint64, u64p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    lib.zsw_set_panel.argtypes = [vp, u8p, u64p, C.c_uint32, C.c_int]
    lib.zsw_score_panel_batch_from.argtypes = [vp, C.POINTER(ZswBatch), C.c_int, C.c_int, u32p, u8p, u8p, u32p, vp]
    lib.zsw_panel_gather_batch.argtypes = [vp, C.POINTER(ZswBatch), u32p, C.c_uint32, u8p, u64p, u32p, C.POINTER(C.c_uint64), vp]
    lib.zsw_panel_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.zsw_debug_panel_records.argtypes = [vp, vp]
    _lib = lib
    return lib
