"""Host-side mirror of the reference's interface for the striped Smith-Waterman path, batched over reads.

Names, argument meaning and error behaviour follow the reference (file:line in the reference checkout):

    ByteIndexMap, DNA_PROFILE_MAP        src/data/constants/mappings/byte_index.rs:231-358, dna.rs:177-178
    WeightMatrix                         src/data/matrices/mod.rs:230-546
    ProfileError / validate_profile_args src/alignment/errors.rs:6-15, profile.rs:32-44
    StripedProfile::{new,sw_score,sw_score_ends,sw_align}   src/alignment/profile.rs:239-519
    LocalProfiles::new_with_w{128,256,512} + ProfileSets    src/alignment/profile_set.rs:71-179,434-483
    MaybeAligned                         src/alignment/types/output.rs:18-25
    SeqSrc                               src/alignment/mod.rs:161-190

The reference builds one profile from one sequence and aligns it against many; here a *batch* of reads
plays the profile role (sw/mod.rs:119-120: the profile is built from the query) and every call runs all
of them against one reference on the GPU through the C ABI (include/zoe_sw.h).  PyTorch is used only
to own device memory and streams.  There is no CPU path in this package.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _lib

SOME, OVERFLOWED, UNMAPPED, EMPTY = 0, 1, 2, 3
BELOW_MIN_SCORE = 4  # only while SwContext.set_min_score(T > 0) is in force: the read scores less than T (include/zoe_sw.h)


class ProfileError(ValueError):
    """src/alignment/errors.rs:6-15"""

    NAMES = {1: "EmptySequence", 2: "GapOpenOutOfRange", 3: "GapExtendOutOfRange", 4: "BadGapWeights"}

    def __init__(self, code: int):
        self.code = code
        self.variant = self.NAMES[code]
        super().__init__(self.variant)


def validate_profile_args(seq_len: int, gap_open: int, gap_extend: int) -> None:
    """src/alignment/profile.rs:32-44"""
    if seq_len == 0:
        raise ProfileError(1)
    if not -127 <= gap_open <= 0:
        raise ProfileError(2)
    if not -127 <= gap_extend <= 0:
        raise ProfileError(3)
    if gap_extend < gap_open:
        raise ProfileError(4)


class ByteIndexMap:
    """256-entry byte -> residue-index table (byte_index.rs:231-358)."""

    def __init__(self, index_map: np.ndarray, byte_keys: bytes):
        self.index_map = np.ascontiguousarray(index_map, dtype=np.uint8)
        self.byte_keys = bytes(byte_keys)

    @staticmethod
    def new(byte_keys: bytes, catch_all: bytes) -> "ByteIndexMap":
        keys = bytes(byte_keys)
        if len(set(keys)) != len(keys):
            raise ValueError("duplicate byte_keys")
        if catch_all[0] not in keys:
            raise ValueError("The catch_all must be present in the byte_keys.")
        m = np.full(256, keys.index(catch_all[0]), dtype=np.uint8)
        for i, k in enumerate(keys):
            m[k] = i
        return ByteIndexMap(m, keys)

    @staticmethod
    def new_ignoring_case(byte_keys: bytes, catch_all: bytes) -> "ByteIndexMap":
        keys = bytes(byte_keys).upper()
        if len(set(keys)) != len(keys):
            raise ValueError("duplicate byte_keys")
        ca = bytes(catch_all).upper()[0]
        if ca not in keys:
            raise ValueError("The catch_all must be present in the byte_keys.")
        m = np.full(256, keys.index(ca), dtype=np.uint8)
        for i, k in enumerate(keys):
            m[k] = i
            m[bytes([k]).lower()[0]] = i
        return ByteIndexMap(m, keys)

    def add_synonym_ignore_case(self, new_key: bytes, previous_key: bytes) -> "ByteIndexMap":
        m = self.index_map.copy()
        idx = m[previous_key[0]]
        m[bytes(new_key).upper()[0]] = idx
        m[bytes(new_key).lower()[0]] = idx
        return ByteIndexMap(m, self.byte_keys)

    def __len__(self) -> int:
        return len(self.byte_keys)

    def to_index(self, b: int) -> int:
        return int(self.index_map[b])


# dna.rs:177-178
DNA_PROFILE_MAP = ByteIndexMap.new_ignoring_case(b"ACGTN", b"N").add_synonym_ignore_case(b"U", b"T")


class WeightMatrix:
    """weights[ref_residue][query_residue] (matrices/mod.rs:230-235). `bias` is non-zero only for the
    unsigned form produced by to_biased_matrix()."""

    def __init__(self, weights: np.ndarray, mapping: ByteIndexMap, bias: int = 0, signed: bool = True):
        self.weights = np.ascontiguousarray(weights)
        self.mapping = mapping
        self.bias = int(bias)
        self.signed = signed

    @staticmethod
    def new(mapping: ByteIndexMap, matching: int, mismatch: int, ignoring: Optional[bytes]) -> "WeightMatrix":
        S = len(mapping)
        w = np.zeros((S, S), dtype=np.int8)
        skip = None
        if ignoring is not None:
            if ignoring[0] not in mapping.byte_keys:
                raise ValueError("An invalid byte was specified for the ignoring field.")
            skip = mapping.to_index(ignoring[0])
        for i in range(S):
            for j in range(S):
                if skip is not None and (skip == i or skip == j):
                    continue
                w[i, j] = matching if i == j else mismatch
        return WeightMatrix(w, mapping)

    @staticmethod
    def new_custom(mapping: ByteIndexMap, weights) -> "WeightMatrix":
        w = np.asarray(weights, dtype=np.int8)
        S = len(mapping)
        if w.shape != (S, S):
            raise ValueError("weights must be SxS")
        return WeightMatrix(w, mapping)

    @staticmethod
    def new_dna_matrix(matching: int, mismatch: int, ignoring: Optional[bytes]) -> "WeightMatrix":
        return WeightMatrix.new(DNA_PROFILE_MAP, matching, mismatch, ignoring)

    @staticmethod
    def new_biased_dna_matrix(matching: int, mismatch: int, ignoring: Optional[bytes]) -> "WeightMatrix":
        return WeightMatrix.new_dna_matrix(matching, mismatch, ignoring).to_biased_matrix()

    def get_bias(self) -> int:
        return int(min(0, int(self.weights.min())))

    def to_biased_matrix(self) -> "WeightMatrix":
        if not self.signed:
            return self
        b = self.get_bias()
        w = (self.weights.astype(np.int16) - b).astype(np.uint8)
        return WeightMatrix(w, self.mapping, bias=-b, signed=False)

    def signed_weights(self) -> np.ndarray:
        if self.signed:
            return self.weights.astype(np.int8)
        return (self.weights.astype(np.int16) - self.bias).astype(np.int8)

    def get_weight(self, ref_residue: int, query_residue: int) -> int:
        return int(self.weights[self.mapping.to_index(ref_residue)][self.mapping.to_index(query_residue)])


@dataclass(frozen=True)
class SeqSrc:
    """src/alignment/mod.rs:161-166: tells an alignment call which role the non-profile sequence plays."""

    seq: bytes
    is_query: bool

    @staticmethod
    def Reference(seq) -> "SeqSrc":
        return SeqSrc(bytes(seq), False)

    @staticmethod
    def Query(seq) -> "SeqSrc":
        return SeqSrc(bytes(seq), True)


# ------------------------------------------------------------------------------------------------
def _torch():
    import torch

    return torch


class SwContext:
    """One zsw_context per GPU (include/zoe_sw.h). Raises if the HIP library or the device is missing."""

    _cache = {}

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        self.device = device
        h = C.c_void_p()
        rc = self.lib.zsw_create(device, C.byref(h))
        if rc != 0:
            raise _lib.ZswError(rc, "zsw_create: " + self.lib.zsw_last_error_string(None).decode())
        self.h = h
        self._scoring_key = None
        self._ref_key = None

    @classmethod
    def get(cls, device: int = 0) -> "SwContext":
        if device not in cls._cache:
            cls._cache[device] = SwContext(device)
        return cls._cache[device]

    def check(self, rc: int, profile_errors: bool = True):
        if rc == 0:
            return
        if profile_errors and 1 <= rc <= 4:
            raise ProfileError(rc)
        raise _lib.ZswError(rc, self.lib.zsw_last_error_string(self.h).decode())

    def set_scoring(self, matrix: WeightMatrix, gap_open: int, gap_extend: int):
        w = np.ascontiguousarray(matrix.signed_weights(), dtype=np.int8)
        key = (w.tobytes(), matrix.mapping.index_map.tobytes(), gap_open, gap_extend)
        if key == self._scoring_key:
            return
        im = matrix.mapping.index_map
        self.check(self.lib.zsw_set_scoring(self.h, w.ctypes.data, w.shape[0], im.ctypes.data, gap_open, gap_extend))
        self._scoring_key = key

    def set_reference(self, reference) -> None:
        torch = _torch()
        if isinstance(reference, torch.Tensor):
            ref = reference.contiguous()
            key = ("t", ref.data_ptr(), ref.numel())
            if key == self._ref_key:
                return
            mem = _lib.MEM_DEVICE if ref.is_cuda else _lib.MEM_HOST
            self.check(self.lib.zsw_set_reference(self.h, ref.data_ptr(), ref.numel(), mem))
            self._ref_key = None  # tensor contents may change; do not cache
            return
        ref = bytes(reference)
        key = ("b", ref)
        if key == self._ref_key:
            return
        buf = np.frombuffer(ref, dtype=np.uint8) if ref else np.zeros(1, dtype=np.uint8)
        self.check(self.lib.zsw_set_reference(self.h, buf.ctypes.data, len(ref), _lib.MEM_HOST))
        self._ref_key = key

    def stream(self) -> int:
        torch = _torch()
        return int(torch.cuda.current_stream(self.device).cuda_stream)

    def parse_sam(self, d_text, n_bytes: Optional[int] = None, final: bool = True, qual_forward: bool = True, rname=None, ref_len: int = 0):
        """zsw_sam_parse_batch over SAM text in device memory (a CUDA uint8 tensor): a sizing call, then the call with arrays of exactly
        the reported sizes. -> (a dict of CUDA tensors: bases, quals, offsets, qnames, qname_offsets (int64), aln (uint8, ALN_DTYPE
        records), status, inc (int32), op, strand, parsed (uint8, PARSED_DTYPE records); the report as numpy uint64). A reader error is
        not raised here: report[SAMTEXT_INFO_ERROR]; the arrays hold the records in front of the failing line."""
        torch = _torch()
        n = int(d_text.numel() if n_bytes is None else n_bytes)
        if not (d_text.is_cuda and d_text.dtype == torch.uint8 and d_text.is_contiguous() and d_text.numel() >= n):
            raise ValueError("d_text: a contiguous CUDA uint8 tensor of at least n_bytes entries")
        dev = d_text.device
        flags = (_lib.SAMTEXT_FINAL if final else 0) | (_lib.SAMTEXT_QUAL_FORWARD if qual_forward else 0)
        rname_b = None if rname is None else (rname.encode() if isinstance(rname, str) else bytes(rname))
        info = (C.c_uint64 * _lib.SAMTEXT_INFO_WORDS)()
        o = _lib.ZswSamParseOut()
        head = (self.h, d_text.data_ptr() if n else None, n, _lib.MEM_DEVICE, flags, rname_b, len(rname_b) if rname_b else 0, int(ref_len))
        self.check(self.lib.zsw_sam_parse_batch(*head, C.byref(o), info, self.stream()), profile_errors=False)
        n_rec, n_bases, n_names, n_cig = (int(info[k]) for k in (_lib.SAMTEXT_INFO_RECORDS, _lib.SAMTEXT_INFO_BASES, _lib.SAMTEXT_INFO_NAME_BYTES,
                                                                 _lib.SAMTEXT_INFO_CIGLETS))
        new = lambda count, dt: torch.empty(max(count, 1), dtype=dt, device=dev)
        t = {"bases": new(n_bases, torch.uint8), "quals": new(n_bases, torch.uint8), "offsets": new(n_rec + 1, torch.int64), "qnames": new(n_names, torch.uint8),
             "qname_offsets": new(n_rec + 1, torch.int64), "aln": new(n_rec * ALN_DTYPE.itemsize, torch.uint8), "status": new(n_rec, torch.uint8),
             "inc": new(n_cig, torch.int32), "op": new(n_cig, torch.uint8), "strand": new(n_rec, torch.uint8),
             "parsed": new(n_rec * PARSED_DTYPE.itemsize, torch.uint8)}
        for k, v in t.items():
            setattr(o, k, v.data_ptr())
        o.base_cap, o.name_cap, o.ciglet_cap, o.record_cap = n_bases, n_names, n_cig, n_rec
        self.check(self.lib.zsw_sam_parse_batch(*head, C.byref(o), info, self.stream()), profile_errors=False)
        sizes = {"bases": n_bases, "quals": n_bases, "offsets": n_rec + 1, "qnames": n_names, "qname_offsets": n_rec + 1, "aln": n_rec * ALN_DTYPE.itemsize,
                 "status": n_rec, "inc": n_cig, "op": n_cig, "strand": n_rec, "parsed": n_rec * PARSED_DTYPE.itemsize}
        return {k: v[:sizes[k]] for k, v in t.items()}, np.array(list(info), dtype=np.uint64)

    def selftest(self):
        self.check(self.lib.zsw_selftest(self.h), profile_errors=False)

    def debug_set(self, flags: int = 0):
        """zsw_debug_set: kernel-selection overrides (_lib.DEBUG_*) for the parity tests; 0 restores the defaults."""
        self.check(self.lib.zsw_debug_set(self.h, int(flags)))

    def debug_band_records(self, records=None):
        """zsw_debug_band_records (tests): the banded seeded pass writes 8 int32 per read — the values its decision rests on —
        into `records` (a CUDA int32 tensor of 8 * n_reads elements that the caller keeps alive); None switches it off."""
        if records is not None:
            assert records.is_cuda and records.dtype == _torch().int32 and records.is_contiguous()
        self._band_records = records
        self.check(self.lib.zsw_debug_band_records(self.h, C.c_void_p(records.data_ptr() if records is not None else None)))

    def debug_cert_records(self, records=None):
        """zsw_debug_cert_records (tests): the certificate pass of the alignment calls writes 4 int32 per read — verdict class,
        deciding parameter, tie count, decided by the sweep launch — into `records` (a CUDA int32 tensor of 4 * n_reads elements
        that the caller keeps alive); None switches it off."""
        if records is not None:
            assert records.is_cuda and records.dtype == _torch().int32 and records.is_contiguous()
        self._cert_records = records
        self.check(self.lib.zsw_debug_cert_records(self.h, C.c_void_p(records.data_ptr() if records is not None else None)))

    def debug_threepass_records(self, records=None):
        """zsw_debug_threepass_records (tests): the third pass of the 3-pass alignment calls writes 8 int32 per read — route,
        accepted band, banded attempts, launch, why the first DP launch handed the read to the rerun, the band that did not fit,
        slot bytes, ciglets — into `records` (a CUDA int32 tensor of 8 * n_reads elements that the caller keeps alive); None
        switches it off."""
        if records is not None:
            assert records.is_cuda and records.dtype == _torch().int32 and records.is_contiguous()
        self._threepass_records = records
        self.check(self.lib.zsw_debug_threepass_records(self.h, C.c_void_p(records.data_ptr() if records is not None else None)))

    def debug_strand_records(self, records=None):
        """zsw_debug_strand_records (tests): the strand-aware calls write 8 int32 per read — support of the anchor vote forward /
        reverse, whole-reference bound forward / reverse (-1: none), the strand that ran first, 1 = settled by proof, 0, 0 — into
        `records` (a CUDA int32 tensor of 8 * n_reads elements that the caller keeps alive); None switches it off."""
        if records is not None:
            assert records.is_cuda and records.dtype == _torch().int32 and records.is_contiguous()
        self._strand_records = records
        self.check(self.lib.zsw_debug_strand_records(self.h, C.c_void_p(records.data_ptr() if records is not None else None)))

    def debug_score_launches(self):
        """zsw_debug_score_launches (tests): the score kernels the last call launched, as a list of (kind, G, C, mode) tuples in
        launch order — kind is a _lib.LAUNCH_* value, (G, C) the strip configuration, mode the MODE the kernel was built with. A
        _lib.LAUNCH_ROW_CHUNKS record is (kind, rows per chunk, rows of overlap, chunks) of the row-chunked launch recorded next."""
        n = C.c_uint32(0)
        self.check(self.lib.zsw_debug_score_launches(self.h, None, 0, C.byref(n)))
        rec = np.zeros((n.value, 4), dtype=np.uint32)
        if n.value:
            self.check(self.lib.zsw_debug_score_launches(self.h, C.c_void_p(rec.ctypes.data), n.value, C.byref(n)))
        return [tuple(int(v) for v in r) for r in rec[: n.value]]

    def set_complement(self, table=None):
        """zsw_set_complement: table[b] = the byte of the base complementary to byte b (256 entries: bytes or a uint8 array);
        None restores the default, the IUPAC nucleotide complement with the case preserved."""
        if table is None:
            self.check(self.lib.zsw_set_complement(self.h, None))
            return
        t = np.ascontiguousarray(np.frombuffer(bytes(table), dtype=np.uint8) if isinstance(table, (bytes, bytearray)) else table, dtype=np.uint8)
        if t.size != 256:
            raise ValueError("a complement table has 256 entries")
        self.check(self.lib.zsw_set_complement(self.h, t.ctypes.data))

    def orient(self, reads: "ReadBatch", strand) -> "ReadBatch":
        """zsw_orient_batch: a ReadBatch of the same layout with every read of strand[i] != 0 replaced by its reverse complement
        (`Nucleotides::to_reverse_complement`); `strand`: a CUDA uint8 tensor with one entry per read."""
        torch = _torch()
        assert strand.is_cuda and strand.dtype == torch.uint8 and strand.numel() >= reads.n_reads
        strand = strand.contiguous()
        out = torch.empty_like(reads.bases)
        b = reads.c_batch()
        self.check(self.lib.zsw_orient_batch(self.h, C.byref(b), strand.data_ptr(), out.data_ptr(), self.stream()))
        return ReadBatch(out, reads.n_reads, fixed_len=reads.fixed_len, offsets=reads.offsets, min_len=reads.min_len)

    def strand_counts(self):
        """zsw_strand_counts of the last strand-aware call: (settled forward by proof, settled reverse by proof, scored on both
        strands, answered as reverse)."""
        c = (C.c_uint64 * 4)()
        self.check(self.lib.zsw_strand_counts(self.h, c))
        return tuple(int(x) for x in c)

    def set_panel(self, seqs) -> int:
        """zsw_set_panel: the members of a reference panel (1 .. _lib.PANEL_MAX_REFS non-empty sequences), independent of
        `set_reference`. `seqs`: a list of byte strings, or the `FastaDeviceBatch` of `records.fasta_batch_from_text` — every record a
        member, taken from device memory where it lies. Returns the number of members."""
        if hasattr(seqs, "bases") and hasattr(seqs, "offsets") and hasattr(seqs, "n_records"):
            n = int(seqs.n_records)
            bases, off = seqs.bases.contiguous(), seqs.offsets.contiguous()
            assert bases.is_cuda and off.is_cuda and off.dtype == _torch().int64 and off.numel() >= n + 1
            self.check(self.lib.zsw_set_panel(self.h, bases.data_ptr(), off.data_ptr(), n, _lib.MEM_DEVICE), profile_errors=False)
            self._panel_size = n
            return n
        seqs = [bytes(s) for s in seqs]
        cat = np.frombuffer(b"".join(seqs) or b"\0", dtype=np.uint8)
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        self.check(self.lib.zsw_set_panel(self.h, cat.ctypes.data, off.ctypes.data, len(seqs), _lib.MEM_HOST), profile_errors=False)
        self._panel_size = len(seqs)
        return len(seqs)

    def panel_counts(self):
        """zsw_panel_counts of the last panel call: (reads settled after one score, (read, member) pairs scored in the first round,
        pairs scored in the second round, reads scored against every member)."""
        c = (C.c_uint64 * 4)()
        self.check(self.lib.zsw_panel_counts(self.h, c))
        return tuple(int(x) for x in c)

    def debug_panel_records(self, records=None):
        """zsw_debug_panel_records (tests): the panel call writes 2 + 2 * n_refs int32 per read — the first-choice member, 1 = settled
        after one score, the n_refs supports of the anchor vote, the n_refs whole-reference bounds (-1: none) — into `records` (a
        CUDA int32 tensor of (2 + 2 * n_refs) * n_reads elements that the caller keeps alive); None switches it off."""
        if records is not None:
            assert records.is_cuda and records.dtype == _torch().int32 and records.is_contiguous()
        self._panel_records = records
        self.check(self.lib.zsw_debug_panel_records(self.h, C.c_void_p(records.data_ptr() if records is not None else None)))

    def panel_gather(self, reads: "ReadBatch", ref_of, k: int):
        """zsw_panel_gather_batch: (the reads with ref_of[i] == k as a ReadBatch of the input's layout, in input order; a CUDA int32
        tensor with the input read each of them is). `ref_of`: a CUDA int32 tensor with one entry per read, e.g. `ScoreBatch.ref`."""
        torch = _torch()
        assert ref_of.is_cuda and ref_of.dtype == torch.int32 and ref_of.numel() >= reads.n_reads
        ref_of = ref_of.contiguous()
        n = reads.n_reads
        dev = reads.bases.device
        out = torch.empty_like(reads.bases)
        index = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev) if reads.offsets is not None else None
        m = C.c_uint64(0)
        b = reads.c_batch()
        self.check(self.lib.zsw_panel_gather_batch(self.h, C.byref(b), ref_of.data_ptr(), int(k), out.data_ptr(), off.data_ptr() if off is not None else None,
                                                   index.data_ptr(), C.byref(m), self.stream()), profile_errors=False)
        m = int(m.value)
        if off is None:
            return ReadBatch(out[:max(m * reads.fixed_len, 1)], m, fixed_len=reads.fixed_len, min_len=reads.fixed_len), index[:m]
        return ReadBatch(out, m, offsets=off[:m + 1]), index[:m]

    def set_profile_sequence(self, sequence: bytes):
        """zsw_set_profile_sequence: the sequence the shared profile is built from (the library itself skips the work when it is the
        one already set: no copy of it is kept on this side, which another binding of the same context could leave stale)"""
        sequence = bytes(sequence)
        buf = (C.c_uint8 * max(len(sequence), 1)).from_buffer_copy(sequence if sequence else b"\0")
        self.check(self.lib.zsw_set_profile_sequence(self.h, buf, len(sequence), _lib.MEM_HOST))

    def set_option(self, option: int, value: int):
        """zsw_set_option, e.g. set_option(_lib.OPTION_EXACT_PRUNING, 0): every cell of every read instead of the seeded exact pass."""
        self.check(self.lib.zsw_set_option(self.h, int(option), int(value)), profile_errors=False)

    def set_min_score(self, t: int):
        """zsw_set_option(ZSW_OPTION_MIN_SCORE, t): reads that score less than t (or are Unmapped) come back with status
        BELOW_MIN_SCORE and every other field 0, settled by the seeded pass's upper bounds where those suffice; every other read is
        what t = 0 (off) returns. Covers the score, ends, ranges and 3-pass calls of the read-as-profile role; the others raise
        ZSW_ERR_UNSUPPORTED while t > 0."""
        self.set_option(_lib.OPTION_MIN_SCORE, int(t))

    def min_score_counts(self):
        """zsw_min_score_counts of the last covered call: reads settled below the minimum (by the whole-read bound, by a band
        bound, by their exact score, in total)."""
        c = (C.c_uint64 * 4)()
        self.check(self.lib.zsw_min_score_counts(self.h, c))
        return tuple(int(x) for x in c)

    def prune_rescored(self) -> int:
        """zsw_prune_rescored: reads the last call's forward seeded (or column-pruned) pass handed back to the full pass
        (the reversed pass of the ranges and alignment calls is not counted; include/zoe_sw.h)."""
        v = C.c_uint64(0)
        self.check(self.lib.zsw_prune_rescored(self.h, C.byref(v)))
        return int(v.value)

    def timing_enable(self, on: bool):
        self.check(self.lib.zsw_timing_enable(self.h, int(on)))

    def timing_read(self):
        s, n = C.c_double(0), C.c_uint64(0)
        self.check(self.lib.zsw_timing_read(self.h, C.byref(s), C.byref(n)))
        return s.value, n.value

    def timing_read_window(self):
        """zsw_timing_read_window: seconds and launches of the seeded pass's window kernel since the last read."""
        s, n = C.c_double(0), C.c_uint64(0)
        self.check(self.lib.zsw_timing_read_window(self.h, C.byref(s), C.byref(n)))
        return s.value, n.value


class SwGroup:
    """zsw_group: several GPUs (or several contexts on one GPU) behind one handle; reads shard into contiguous index ranges,
    one host thread drives each context (include/zoe_sw.h). Host batches get their results in place; device shards are
    completed on every device by one RCCL all-gather."""

    def __init__(self, device_ids: Sequence[int]):
        self.lib = _lib.load()
        self.devices = [int(d) for d in device_ids]
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        rc = self.lib.zsw_group_create(arr, len(self.devices), C.byref(h))
        if rc != 0:
            raise _lib.ZswError(rc, "zsw_group_create: " + self.lib.zsw_last_error_string(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.zsw_group_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def check(self, rc: int):
        if rc == 0:
            return
        if 1 <= rc <= 4:
            raise ProfileError(rc)
        raise _lib.ZswError(rc, self.lib.zsw_group_last_error_string(self.h).decode())

    def __len__(self):
        return int(self.lib.zsw_group_size(self.h))

    def configure(self, matrix: WeightMatrix, gap_open: int, gap_extend: int, reference: bytes):
        w = np.ascontiguousarray(matrix.signed_weights(), dtype=np.int8)
        im = matrix.mapping.index_map
        self.check(self.lib.zsw_group_set_scoring(self.h, w.ctypes.data, w.shape[0], im.ctypes.data, gap_open, gap_extend))
        ref = np.frombuffer(bytes(reference), dtype=np.uint8) if len(reference) else np.zeros(1, dtype=np.uint8)
        self.check(self.lib.zsw_group_set_reference(self.h, ref.ctypes.data, len(reference)))

    def sw_score_from_host(self, bases: np.ndarray, n_reads: int, fixed_len: int = 0, offsets: Optional[np.ndarray] = None,
                           width: int = 8, preset: int = 256):
        """ProfileSets::sw_score_from_i{width} for a batch in host memory; returns (score u32, status u8, tier u8) numpy arrays."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        b = _lib.ZswBatch()
        b.bases = bases.ctypes.data
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.uint64)
            b.offsets = off.ctypes.data
        b.fixed_len = int(fixed_len)
        b.n_reads = int(n_reads)
        b.mem = _lib.MEM_HOST
        score = np.zeros(max(n_reads, 1), dtype=np.uint32)
        status = np.zeros(max(n_reads, 1), dtype=np.uint8)
        tier = np.zeros(max(n_reads, 1), dtype=np.uint8)
        self.check(self.lib.zsw_group_score_batch_from(self.h, C.byref(b), width, preset, score.ctypes.data, status.ctypes.data, tier.ctypes.data))
        return score[:n_reads], status[:n_reads], tier[:n_reads]

    def sw_align_from_host(self, bases: np.ndarray, n_reads: int, fixed_len: int = 0, offsets: Optional[np.ndarray] = None,
                           width: int = 8, preset: int = 256, invert: bool = False, three_pass: bool = False) -> "AlignmentBatch":
        """ProfileSets::sw_align_from_i{width} (or its _3pass form) for a batch in host memory, sharded over the group."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        b = _lib.ZswBatch()
        b.bases = bases.ctypes.data
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.uint64)
            b.offsets = off.ctypes.data
        b.fixed_len = int(fixed_len)
        b.n_reads = int(n_reads)
        b.mem = _lib.MEM_HOST
        n = int(n_reads)
        rec = np.zeros(max(n, 1), dtype=ALN_DTYPE)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        tier = np.zeros(max(n, 1), dtype=np.uint8)
        fn = self.lib.zsw_group_align_3pass_batch_from if three_pass else self.lib.zsw_group_align_batch_from
        cap = max(8 * n, 64)
        total = C.c_uint64(0)
        while True:
            inc = np.zeros(cap, dtype=np.uint32)
            op = np.zeros(cap, dtype=np.uint8)
            rc = fn(self.h, C.byref(b), width, preset, int(invert), rec.ctypes.data, status.ctypes.data, tier.ctypes.data,
                    inc.ctypes.data, op.ctypes.data, cap, C.byref(total))
            if rc == -1 and total.value > cap:
                cap = int(total.value)
                continue
            self.check(rc)
            break
        t = int(total.value)
        return AlignmentBatch(status[:n], rec[:n], inc[:t], op[:t], tier[:n])

    def sw_score_from_device(self, shards: Sequence["ReadBatch"], width: int = 8, preset: int = 256):
        """One device-resident ReadBatch per context; returns per device the (score, status) tensors of ALL reads in shard order."""
        torch = _torch()
        if len(shards) != len(self.devices):
            raise ValueError("one shard per context")
        total = sum(s.n_reads for s in shards)
        arr = (_lib.ZswBatch * len(shards))(*[s.c_batch() for s in shards])
        outs = [(torch.zeros(max(total, 1), dtype=torch.int32, device=s.bases.device), torch.zeros(max(total, 1), dtype=torch.uint8, device=s.bases.device))
                for s in shards]
        ps = (C.c_void_p * len(shards))(*[o[0].data_ptr() for o in outs])
        pt = (C.c_void_p * len(shards))(*[o[1].data_ptr() for o in outs])
        torch.cuda.synchronize()
        self.check(self.lib.zsw_group_score_batch_from_device(self.h, arr, width, preset, ps, pt))
        return [(o[0][:total], o[1][:total]) for o in outs]


class ReadBatch:
    """Device-resident reads: `bases` uint8 (concatenated), and either `fixed_len` or `offsets` (int64[n+1])."""

    def __init__(self, bases, n_reads: int, fixed_len: int = 0, offsets=None, min_len: Optional[int] = None):
        self.bases = bases
        self.n_reads = int(n_reads)
        self.fixed_len = int(fixed_len)
        self.offsets = offsets
        self.min_len = min_len  # known on the host when built from host data

    @staticmethod
    def from_sequences(seqs: Sequence[bytes], device: int = 0) -> "ReadBatch":
        torch = _torch()
        lens = [len(s) for s in seqs]
        dev = torch.device("cuda", device)
        cat = b"".join(bytes(s) for s in seqs)
        bases = torch.frombuffer(bytearray(cat if cat else b"\0"), dtype=torch.uint8).to(dev)
        if lens and all(l == lens[0] for l in lens) and lens[0] > 0:
            return ReadBatch(bases, len(seqs), fixed_len=lens[0], min_len=lens[0])
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        return ReadBatch(bases, len(seqs), offsets=torch.from_numpy(off).to(dev), min_len=min(lens) if lens else None)

    @staticmethod
    def from_fixed(bases, fixed_len: int) -> "ReadBatch":
        return ReadBatch(bases, bases.numel() // fixed_len, fixed_len=fixed_len, min_len=fixed_len)

    def c_batch(self) -> _lib.ZswBatch:
        b = _lib.ZswBatch()
        b.bases = self.bases.data_ptr()
        b.offsets = self.offsets.data_ptr() if self.offsets is not None else None
        b.fixed_len = self.fixed_len
        b.n_reads = self.n_reads
        b.mem = _lib.MEM_DEVICE
        b.encoding = 0
        return b

    @property
    def device_index(self) -> int:
        return self.bases.device.index or 0


@dataclass
class ScoreBatch:
    """MaybeAligned<u32> per read: status (SOME/OVERFLOWED/UNMAPPED/EMPTY, BELOW_MIN_SCORE under SwContext.set_min_score) +
    score (valid where SOME)."""

    score: "object"
    status: "object"
    tier: Optional["object"] = None
    ref_end: Optional["object"] = None
    query_end: Optional["object"] = None
    ref_start: Optional["object"] = None
    query_start: Optional["object"] = None
    strand: Optional["object"] = None  # strand-aware calls: 0 = the read as given, 1 = its reverse complement
    ref: Optional["object"] = None  # panel calls: the member of the panel that answered (int32)

    def maybe_aligned(self, i: int):
        st = int(self.status[i])
        return ("Some", int(self.score[i])) if st == SOME else ({1: "Overflowed", 2: "Unmapped", 3: "Empty", 4: "BelowMinScore"}[st], None)


@dataclass
class AlignmentBatch:
    """MaybeAligned<Alignment<u32>> per read; ciglets flattened (inc, op) with per-read offsets. A read below the context's
    minimum score (status BELOW_MIN_SCORE) has a zeroed record and no ciglets, like an UNMAPPED one."""

    status: np.ndarray
    records: np.ndarray  # structured: score, ref_start, ref_end, query_start, query_end, ref_len, query_len, n_ciglets, ciglet_offset
    inc: np.ndarray
    op: np.ndarray
    tier: Optional[np.ndarray] = None
    strand: Optional[np.ndarray] = None  # strand-aware calls: 0 = the read as given, 1 = its reverse complement (coordinates are its)

    def cigar(self, i: int) -> str:
        r = self.records[i]
        o, n = int(r["ciglet_offset"]), int(r["n_ciglets"])
        return "".join(f"{int(self.inc[o + k])}{chr(int(self.op[o + k]))}" for k in range(n))

    def key(self, i: int):
        st = int(self.status[i])
        if st != SOME:
            return (st, 0, (0, 0), (0, 0), "", 0, 0)
        r = self.records[i]
        return (st, int(r["score"]), (int(r["ref_start"]), int(r["ref_end"])), (int(r["query_start"]), int(r["query_end"])),
                self.cigar(i), int(r["ref_len"]), int(r["query_len"]))

    @staticmethod
    def nm(stats: np.ndarray) -> np.ndarray:
        """The NM tag of SAM per read, from the stats array of `annotate`: mismatches + inserted + deleted bases."""
        return stats["mismatches"] + stats["ins_bases"] + stats["del_bases"]


ALN_DTYPE = np.dtype(
    [("score", "<u4"), ("ref_start", "<u4"), ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"),
     ("ref_len", "<u4"), ("query_len", "<u4"), ("n_ciglets", "<u4"), ("ciglet_offset", "<u8")]
)

# zsw_sam_parsed: what zsw_sam_parse_batch keeps of a SAM line beside its record
PARSED_DTYPE = np.dtype([("pos", "<u8"), ("line", "<u8"), ("flag", "<u2"), ("mapq", "u1"), ("code", "u1"), ("bits", "<u4")])

# zsw_alignment_stats: what zsw_annotate_batch counts along one CIGAR (path_status: a _lib.PATH_* value)
STATS_DTYPE = np.dtype([("matches", "<u4"), ("mismatches", "<u4"), ("ins_bases", "<u4"), ("del_bases", "<u4"), ("ins_runs", "<u4"), ("del_runs", "<u4"),
                        ("path_score", "<i4"), ("path_status", "<u4")])


def _annotate(ctx: "SwContext", rb: "ReadBatch", aln: AlignmentBatch, flags: int, verbose: bool):
    """zsw_annotate_batch over the records of `aln` (host arrays: they are uploaded), with the context configured by the caller.
    -> (the verbose AlignmentBatch or None, stats as STATS_DTYPE)"""
    torch = _torch()
    n, dev = rb.n_reads, rb.bases.device
    if len(aln.status) != n:
        raise ValueError("the alignments are not those of this batch of reads")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy() if a.size else np.zeros(1, dtype=dt)).to(dev)
    d_aln, d_status = up(aln.records, np.uint8), up(aln.status, np.uint8)
    d_inc, d_op = up(aln.inc, np.int32), up(aln.op, np.uint8)
    t_in = int(aln.inc.size)
    stats = torch.zeros(max(n, 1) * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    b = rb.c_batch()
    if not verbose:
        ctx.check(ctx.lib.zsw_annotate_batch(ctx.h, C.byref(b), flags, d_aln.data_ptr(), d_status.data_ptr(), d_inc.data_ptr(), d_op.data_ptr(), t_in,
                                             stats.data_ptr(), None, None, None, 0, None, ctx.stream()), profile_errors=False)
        torch.cuda.synchronize(dev)
        return None, _to_host(stats[: n * STATS_DTYPE.itemsize])[0].view(STATS_DTYPE)
    out = torch.zeros(max(n, 1) * ALN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    cap = max(2 * t_in, 64)
    total = C.c_uint64(0)
    while True:
        inc = torch.empty(cap, dtype=torch.int32, device=dev)
        op = torch.empty(cap, dtype=torch.uint8, device=dev)
        rc = ctx.lib.zsw_annotate_batch(ctx.h, C.byref(b), flags, d_aln.data_ptr(), d_status.data_ptr(), d_inc.data_ptr(), d_op.data_ptr(), t_in,
                                        stats.data_ptr(), out.data_ptr(), inc.data_ptr(), op.data_ptr(), cap, C.byref(total), ctx.stream())
        if rc == -1 and total.value > cap:
            cap = int(total.value)
            continue
        ctx.check(rc, profile_errors=False)
        break
    torch.cuda.synchronize(dev)
    t = int(total.value)
    h_stats, h_out, h_inc, h_op = _to_host(stats[: n * STATS_DTYPE.itemsize], out[: n * ALN_DTYPE.itemsize], inc[:t], op[:t])
    return AlignmentBatch(aln.status, h_out.view(ALN_DTYPE), h_inc.view(np.uint32), h_op, aln.tier, aln.strand), h_stats.view(STATS_DTYPE)


def _pileup(ctx: "SwContext", rb: "ReadBatch", aln: AlignmentBatch, flags: int, seq_len: int, counts, insertions: bool):
    """zsw_pileup_batch over the records of `aln` (host arrays: they are uploaded), with the sequence the flags name set on the context
    by the caller. counts: None (a new table) or the (seq_len, 8) CUDA int32 tensor of an earlier call, which is added to.
    -> the table, or with `insertions` (the table, a (seq_len + 1, 2) CUDA int32 tensor of runs and bases in front of each position)"""
    torch = _torch()
    n, dev = rb.n_reads, rb.bases.device
    if len(aln.status) != n:
        raise ValueError("the alignments are not those of this batch of reads")
    if counts is None:
        counts = torch.zeros((seq_len, len(_lib.PILEUP_BINS)), dtype=torch.int32, device=dev)
    elif not (counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (seq_len, 8)):
        raise ValueError("counts: the contiguous (len, 8) CUDA int32 tensor of an earlier pileup over this sequence")
    ins = torch.zeros((seq_len + 1, 2), dtype=torch.int32, device=dev) if insertions else None
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy() if a.size else np.zeros(1, dtype=dt)).to(dev)
    d_aln, d_status = up(aln.records, np.uint8), up(aln.status, np.uint8)
    d_inc, d_op = up(aln.inc, np.int32), up(aln.op, np.uint8)
    b = rb.c_batch()
    n_bad = C.c_uint64(0)
    ctx.check(ctx.lib.zsw_pileup_batch(ctx.h, C.byref(b), flags, d_aln.data_ptr(), d_status.data_ptr(), d_inc.data_ptr(), d_op.data_ptr(), int(aln.inc.size),
                                       counts.data_ptr() if seq_len else None, ins.data_ptr() if insertions else None, C.byref(n_bad), ctx.stream()),
              profile_errors=False)
    torch.cuda.synchronize(dev)
    if n_bad.value:
        raise ValueError(f"{n_bad.value} records are not alignments of these reads to this sequence")
    return (counts, ins) if insertions else counts


def plurality_acgtn(counts, fallback=None):
    """zsw_consensus_from_counts: `CreateConsensus::plurality_acgtn` of a (len, 8) table of `pileup` — per site the most frequent of
    A C G T N, ties in that order, so `A` where nothing was counted. fallback (bytes, or a CUDA uint8 tensor of len entries): sites
    without any A C G T N count take its byte instead. counts on a GPU -> a CUDA uint8 tensor, which `SwContext.set_reference`
    takes as it is (zsw_set_reference with ZSW_MEM_DEVICE); a numpy array -> bytes."""
    torch = _torch()
    host = not isinstance(counts, torch.Tensor)
    if host:
        t = np.ascontiguousarray(counts, dtype=np.uint32)
        device = 0
    else:
        t = counts.contiguous()
        if not t.is_cuda or t.dtype != torch.int32:
            raise ValueError("counts: a CUDA int32 tensor or a numpy array")
        device = t.device.index
    if t.ndim != 2 or t.shape[1] != 8:
        raise ValueError("counts: (len, 8)")
    n = int(t.shape[0])
    ctx = SwContext.get(device)
    flags = _lib.CONSENSUS_KEEP_UNCOVERED if fallback is not None else 0
    if host:
        fb = np.frombuffer(bytes(fallback), dtype=np.uint8) if fallback is not None else None
        out = np.zeros(max(n, 1), dtype=np.uint8)
        if fb is not None and fb.size != n:
            raise ValueError("fallback: one byte per site")
        ctx.check(ctx.lib.zsw_consensus_from_counts(ctx.h, t.ctypes.data if n else None, n, _lib.MEM_HOST, flags, fb.ctypes.data if fb is not None and n else None,
                                                    out.ctypes.data, None), profile_errors=False)
        return out[:n].tobytes()
    if fallback is not None and not isinstance(fallback, torch.Tensor):
        fallback = torch.from_numpy(np.frombuffer(bytes(fallback), dtype=np.uint8).copy()).to(t.device)
    if fallback is not None and (fallback.numel() != n or fallback.dtype != torch.uint8 or not fallback.is_cuda):
        raise ValueError("fallback: one byte per site")
    out = torch.empty(max(n, 1), dtype=torch.uint8, device=t.device)
    ctx.check(ctx.lib.zsw_consensus_from_counts(ctx.h, t.data_ptr() if n else None, n, _lib.MEM_DEVICE, flags, fallback.contiguous().data_ptr() if fallback is not None and n else None,
                                                out.data_ptr(), ctx.stream()), profile_errors=False)
    return out[:n]


def _sam_text(ctx: "SwContext", rb: "ReadBatch", aln: AlignmentBatch, qnames, quals, rname, mapq: int, strands, stats, omit_seq: bool, device_out: bool):
    """zsw_sam_batch over the records of `aln` (host arrays: they are uploaded) beside the reads `rb` as aligned.
    -> bytes, or with device_out (a CUDA uint8 tensor with the text, a CUDA int64 tensor with the n + 1 line offsets)"""
    torch = _torch()
    n, dev = rb.n_reads, rb.bases.device
    if len(aln.status) != n:
        raise ValueError("the alignments are not those of this batch of reads")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy() if a.size else np.zeros(1, dtype=dt)).to(dev)
    d_aln, d_status = up(aln.records, np.uint8), up(aln.status, np.uint8)
    d_inc, d_op = up(aln.inc, np.int32), up(aln.op, np.uint8)
    keep = [d_aln, d_status, d_inc, d_op]
    f = _lib.ZswSamFields()
    if isinstance(qnames, tuple) and len(qnames) == 2 and isinstance(qnames[0], torch.Tensor):  # (names back to back, n + 1 offsets) on the device
        d_names, d_noff = qnames[0].contiguous(), qnames[1].contiguous()
        if not (d_names.is_cuda and d_noff.is_cuda) or d_names.dtype != torch.uint8 or d_noff.dtype != torch.int64 or d_noff.numel() < n + 1:
            raise ValueError("qnames: a CUDA uint8 tensor of the names and a CUDA int64 tensor of n + 1 offsets")
        keep += [d_names, d_noff]
        f.qnames, f.qname_offsets = d_names.data_ptr(), d_noff.data_ptr()
    elif qnames is not None:
        names = [q.encode() if isinstance(q, str) else bytes(q) for q in qnames]
        if len(names) != n:
            raise ValueError("one QNAME per read")
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(q) for q in names], out=off[1:])
        d_names, d_noff = up(np.frombuffer(b"".join(names), dtype=np.uint8), np.uint8), up(off, np.int64)
        keep += [d_names, d_noff]
        f.qnames, f.qname_offsets = d_names.data_ptr(), d_noff.data_ptr()
    if quals is not None:
        if isinstance(quals, torch.Tensor):  # laid out as the reads' bases
            d_quals = quals.contiguous()
            if not d_quals.is_cuda or d_quals.dtype != torch.uint8 or d_quals.numel() < rb.bases.numel():
                raise ValueError("quals: a CUDA uint8 tensor laid out as the reads' bases")
        else:
            q = b"".join(bytes(x) for x in quals)
            lens = np.fromiter((len(x) for x in quals), dtype=np.int64, count=len(quals))
            want = np.full(n, rb.fixed_len, dtype=np.int64) if rb.offsets is None else np.diff(_to_host(rb.offsets)[0][: n + 1])
            if len(lens) != n or not np.array_equal(lens, want):
                raise ValueError("one quality string per read, as long as the read")
            d_quals = up(np.frombuffer(q, dtype=np.uint8), np.uint8)
        keep.append(d_quals)
        f.quals = d_quals.data_ptr()
    if strands is not None:
        d_strand = up(np.asarray(strands, dtype=np.uint8), np.uint8)
        if d_strand.numel() < n:
            raise ValueError("one strand per read")
        keep.append(d_strand)
        f.strand = d_strand.data_ptr()
    if stats is not None:
        if stats.dtype != STATS_DTYPE or len(stats) != n:
            raise ValueError("stats: the STATS_DTYPE array of `annotate` for this batch")
        d_stats = up(stats, np.uint8)
        keep.append(d_stats)
        f.stats = d_stats.data_ptr()
    rname_b = rname.encode() if isinstance(rname, str) else bytes(rname)
    f.rname, f.rname_len, f.mapq = rname_b, len(rname_b), int(mapq)
    flags = _lib.SAM_OMIT_SEQ if omit_seq else 0
    b = rb.c_batch()
    total, n_bad = C.c_uint64(0), C.c_uint64(0)
    t_in = int(aln.inc.size)
    args = (ctx.h, C.byref(b), C.byref(f), flags, d_aln.data_ptr(), d_status.data_ptr(), d_inc.data_ptr(), d_op.data_ptr(), t_in)
    ctx.check(ctx.lib.zsw_sam_batch(*args, None, 0, C.byref(total), None, C.byref(n_bad), ctx.stream()), profile_errors=False)
    text = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ctx.check(ctx.lib.zsw_sam_batch(*args, text.data_ptr(), int(total.value), C.byref(total), offsets.data_ptr(), C.byref(n_bad), ctx.stream()), profile_errors=False)
    torch.cuda.synchronize(dev)
    del keep
    text = text[: int(total.value)]
    if device_out:
        return text, offsets
    return _to_host(text)[0].tobytes() if text.numel() else b""


def _to_host(*tensors):
    """Device tensors -> numpy arrays through page-locked buffers (torch caches them between calls), all copies in flight together:
    a 10 M-read alignment hands back half a gigabyte of records and ciglets, which pageable copies move at a fifth of the PCIe rate."""
    torch = _torch()
    out = []
    for t in tensors:
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        out.append(h)
    if tensors:
        torch.cuda.synchronize(tensors[0].device)
    return [h.numpy() for h in out]


def _as_batch(reads, device: int) -> ReadBatch:
    if isinstance(reads, ReadBatch):
        return reads
    return ReadBatch.from_sequences(list(reads), device)


class _ProfileBatchBase:
    def __init__(self, reads, matrix: WeightMatrix, gap_open: int, gap_extend: int, device: int = 0):
        rb = _as_batch(reads, device)
        # validate_profile_args: the sequence check is per read; an empty read known on the host raises here,
        # one only visible on the device comes back with status EMPTY.
        validate_profile_args(1 if rb.min_len is None else rb.min_len, gap_open, gap_extend)
        self.reads = rb
        self.matrix = matrix
        self.gap_open = gap_open
        self.gap_extend = gap_extend
        self.ctx = SwContext.get(rb.device_index)

    def _prep(self, reference):
        self.ctx.set_scoring(self.matrix, self.gap_open, self.gap_extend)
        self.ctx.set_reference(reference)

    def _align(self, seq: SeqSrc, direct, from_width=None, preset=None, three_pass: bool = False, strands: bool = False) -> AlignmentBatch:
        torch = _torch()
        self._prep(seq.seq)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        aln = torch.zeros(max(n, 1) * ALN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        tier = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        strand = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        cap = max(8 * n, 64)  # typical reads need 1-3 ciglets; the call reports the exact total when this is too small
        b = self.reads.c_batch()
        total = C.c_uint64(0)
        while True:
            inc = torch.empty(cap, dtype=torch.int32, device=dev)
            op = torch.empty(cap, dtype=torch.uint8, device=dev)
            fn_direct = self.ctx.lib.zsw_align_3pass_batch if three_pass else self.ctx.lib.zsw_align_batch
            fn_from = self.ctx.lib.zsw_align_3pass_batch_from if three_pass else self.ctx.lib.zsw_align_batch_from
            if strands:  # zsw_align_3pass_strands_batch_from: the cascade's 3-pass call on whichever strand scores higher
                rc = self.ctx.lib.zsw_align_3pass_strands_batch_from(self.ctx.h, C.byref(b), from_width, preset, int(seq.is_query), aln.data_ptr(),
                                                                     status.data_ptr(), tier.data_ptr(), strand.data_ptr(), inc.data_ptr(), op.data_ptr(),
                                                                     cap, C.byref(total), self.ctx.stream())
            elif direct is not None:
                rc = fn_direct(self.ctx.h, C.byref(b), direct[0], direct[1], int(seq.is_query), aln.data_ptr(),
                                                  status.data_ptr(), inc.data_ptr(), op.data_ptr(), cap, C.byref(total), self.ctx.stream())
            else:
                rc = fn_from(self.ctx.h, C.byref(b), from_width, preset, int(seq.is_query), aln.data_ptr(),
                                                       status.data_ptr(), tier.data_ptr(), inc.data_ptr(), op.data_ptr(), cap,
                                                       C.byref(total), self.ctx.stream())
            if rc == -1 and total.value > cap:
                cap = int(total.value)
                continue
            self.ctx.check(rc)
            break
        torch.cuda.synchronize(dev)
        t = int(total.value)
        h_aln, h_status, h_inc, h_op, h_tier = _to_host(aln[: n * ALN_DTYPE.itemsize], status[:n], inc[:t], op[:t], tier[:n])
        out = AlignmentBatch(h_status, h_aln.view(ALN_DTYPE), h_inc.view(np.uint32), h_op, h_tier if direct is None else None)
        if strands:
            out.strand = _to_host(strand[:n])[0]
        return out


    def annotate(self, aln: AlignmentBatch, seq: SeqSrc, residues: bool = False, verbose: bool = True):
        """zsw_annotate_batch over the alignments `aln` that one of this batch's alignment calls returned for `seq` (the same
        SeqSrc): -> (the AlignmentBatch of `Alignment::to_verbose_sequence_matching`, M split into = / X, or None without `verbose`;
        a STATS_DTYPE array: matches, mismatches, gap bases and runs, `sw_score_from_path` and its status per read).
        residues: a column matches when the index map sends both bytes to one residue (default: equal bytes, as the reference).
        Alignments of a strand-aware call are annotated against the reads as aligned (strand 1: the reverse complement)."""
        self._prep(seq.seq)
        reads = self.reads
        if aln.strand is not None:
            reads = self.ctx.orient(reads, _torch().from_numpy(np.ascontiguousarray(aln.strand, dtype=np.uint8)).to(reads.bases.device))
        flags = (_lib.ANNOTATE_READ_IS_REF if seq.is_query else 0) | (_lib.ANNOTATE_MATCH_RESIDUES if residues else 0)
        return _annotate(self.ctx, reads, aln, flags, verbose)

    def pileup(self, aln: AlignmentBatch, seq: SeqSrc, counts=None, insertions: bool = False):
        """zsw_pileup_batch over the alignments `aln` that one of this batch's alignment calls returned for `seq` (the same SeqSrc):
        -> the (len(seq), 8) CUDA int32 table of how often a read byte of each bin — _lib.PILEUP_BINS: A C G T/U N, gap, other IUPAC,
        invalid — stood opposite each position of `seq` (`AlignmentComposition::per_site_counts` in the coordinates of `seq`).
        counts: the table of an earlier call, which is added to (batches accumulate). insertions: also the (len + 1, 2) table of
        insertion runs and bases in front of each position. `plurality_acgtn(counts)` is the consensus. Alignments of a
        strand-aware call are piled up from the reads as aligned (strand 1: the reverse complement)."""
        self._prep(seq.seq)
        reads = self.reads
        if aln.strand is not None:
            reads = self.ctx.orient(reads, _torch().from_numpy(np.ascontiguousarray(aln.strand, dtype=np.uint8)).to(reads.bases.device))
        return _pileup(self.ctx, reads, aln, _lib.ANNOTATE_READ_IS_REF if seq.is_query else 0, len(seq.seq), counts, insertions)

    def to_sam_text(self, aln: AlignmentBatch, qnames, quals=None, rname="ref", mapq: int = 255, strands=None, stats=None, omit_seq: bool = False,
                    device: bool = False):
        """zsw_sam_batch: the SAM body for the alignments `aln` of this batch (those of an alignment call, or the verbose ones of
        `annotate`), one line per read — what `str(SamData.from_alignment(..))` / `str(SamData.unmapped(..))` of zoe_amd/records.py give,
        each closed by a newline — formatted on the GPU. qnames: one name per read, a pair of CUDA tensors (the names back to back, uint8; n + 1
        offsets, int64) as `records.fastq_batch_from_text` leaves them, or None ("*"); quals: the qualities as read, one
        byte string per read or a CUDA uint8 tensor laid out as the reads, or None ("*"); strands: default `aln.strand` — strand 1:
        FLAG 16, SEQ the reverse complement (the reads are oriented as for `annotate`), QUAL reversed; stats: the stats array of
        `annotate`, for NM:i:; omit_seq: SEQ "*". -> bytes, or with `device` (a CUDA uint8 tensor, a CUDA int64 tensor of n + 1 line
        offsets). A read of length 0 has "*" for SEQ and QUAL."""
        strands = aln.strand if strands is None else strands
        reads = self.reads
        if strands is not None:
            reads = self.ctx.orient(reads, _torch().from_numpy(np.ascontiguousarray(strands, dtype=np.uint8)).to(reads.bases.device))
        return _sam_text(self.ctx, reads, aln, qnames, quals, rname, mapq, strands, stats, omit_seq, device)


class StripedProfileBatch(_ProfileBatchBase):
    """`StripedProfile::<T, N, S>::new(read_i, &matrix, gap_open, gap_extend)` for every read of a batch.

    For unsigned T pass matrix.to_biased_matrix() exactly as the reference requires (profile.rs:215-219)."""

    def __init__(self, reads, matrix: WeightMatrix, gap_open: int, gap_extend: int, T: str = "i16", N: int = 16, device: int = 0):
        if T not in _lib.INT_TYPES:
            raise ValueError(f"T must be one of {list(_lib.INT_TYPES)}")
        if T.startswith("u") and matrix.signed:
            raise ValueError("unsigned T needs matrix.to_biased_matrix() (profile.rs:215-219)")
        if T.startswith("i") and not matrix.signed:
            raise ValueError("signed T needs the signed matrix")
        super().__init__(reads, matrix, gap_open, gap_extend, device)
        self.T, self.N = T, N

    new = classmethod(lambda cls, *a, **k: cls(*a, **k))

    def sw_score(self, reference) -> ScoreBatch:
        """profile.rs:440-446 → sw_simd_score (striped.rs:65-142)"""
        torch = _torch()
        self._prep(reference)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        score = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = self.reads.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_batch(self.ctx.h, C.byref(b), _lib.INT_TYPES[self.T], self.N, score.data_ptr(),
                                                    status.data_ptr(), self.ctx.stream()))
        return ScoreBatch(score[:n], status[:n])

    def sw_score_ends(self, seq: SeqSrc) -> ScoreBatch:
        """profile.rs:456-460 → sw_simd_score_ends (striped.rs:153-162). SeqSrc::Query swaps the two ends."""
        torch = _torch()
        self._prep(seq.seq)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        score = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        rend = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        qend = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = self.reads.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_ends_batch(self.ctx.h, C.byref(b), _lib.INT_TYPES[self.T], self.N, score.data_ptr(),
                                                         rend.data_ptr(), qend.data_ptr(), status.data_ptr(), self.ctx.stream()))
        if seq.is_query:
            rend, qend = qend, rend
        return ScoreBatch(score[:n], status[:n], ref_end=rend[:n], query_end=qend[:n])

    def sw_score_ranges(self, seq: SeqSrc) -> ScoreBatch:
        """profile.rs:529-533 → sw_simd_score_ranges (striped.rs:355-388): ScoreAndRanges per read (0-based half-open);
        SeqSrc::Query swaps the reference and query ranges."""
        torch = _torch()
        self._prep(seq.seq)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        o = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for _ in range(5)]
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = self.reads.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_ranges_batch(self.ctx.h, C.byref(b), _lib.INT_TYPES[self.T], self.N, o[0].data_ptr(),
                                                           o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(),
                                                           status.data_ptr(), self.ctx.stream()))
        rs, re_, qs, qe = (x[:n] for x in o[1:])
        if seq.is_query:
            rs, re_, qs, qe = qs, qe, rs, re_
        return ScoreBatch(o[0][:n], status[:n], ref_start=rs, ref_end=re_, query_start=qs, query_end=qe)

    def sw_align(self, seq: SeqSrc) -> AlignmentBatch:
        """profile.rs:515-519 → sw_simd_align (striped.rs:449-598)"""
        return self._align(seq, (_lib.INT_TYPES[self.T], self.N))

    def sw_align_3pass(self, seq: SeqSrc) -> AlignmentBatch:
        """profile.rs:546-552 → sw_align_3pass (three_pass.rs:21-104)"""
        return self._align(seq, (_lib.INT_TYPES[self.T], self.N), three_pass=True)


class LocalProfilesBatch(_ProfileBatchBase):
    """`LocalProfiles::new_with_w{128,256,512}(read_i, &matrix, gap_open, gap_extend)` for every read."""

    def __init__(self, reads, matrix: WeightMatrix, gap_open: int, gap_extend: int, preset: int = 256, device: int = 0):
        if not matrix.signed:
            raise ValueError("profile sets take the signed matrix (profile_set.rs:382-390)")
        if preset not in (128, 256, 512):
            raise ValueError("preset must be 128, 256 or 512")
        super().__init__(reads, matrix, gap_open, gap_extend, device)
        self.preset = preset

    @classmethod
    def new_with_w128(cls, reads, matrix, gap_open, gap_extend, device=0):
        return cls(reads, matrix, gap_open, gap_extend, 128, device)

    @classmethod
    def new_with_w256(cls, reads, matrix, gap_open, gap_extend, device=0):
        return cls(reads, matrix, gap_open, gap_extend, 256, device)

    @classmethod
    def new_with_w512(cls, reads, matrix, gap_open, gap_extend, device=0):
        return cls(reads, matrix, gap_open, gap_extend, 512, device)

    def _score_from(self, reference, width: int, out=None) -> ScoreBatch:
        """`out`: an object with preallocated `score` (int32) and `status` (uint8) device tensors of at least n reads, e.g. a
        zoe_amd.dist.ResultSlab, so that the kernel writes straight into the buffer a collective sends."""
        torch = _torch()
        self._prep(reference)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        if out is not None:
            score, status = out.score, out.status
            if score.numel() < n or status.numel() < n or score.device != dev:
                raise ValueError("out.score / out.status too small or on another device")
        else:
            score = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        tier = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = self.reads.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_batch_from(self.ctx.h, C.byref(b), width, self.preset, score.data_ptr(),
                                                         status.data_ptr(), tier.data_ptr(), self.ctx.stream()))
        return ScoreBatch(score[:n], status[:n], tier=tier[:n])

    def sw_score_from_i8(self, reference, out=None) -> ScoreBatch:
        return self._score_from(reference, 8, out)

    def sw_score_from_i16(self, reference) -> ScoreBatch:
        return self._score_from(reference, 16)

    def sw_score_from_i32(self, reference) -> ScoreBatch:
        return self._score_from(reference, 32)

    def _score_strands_from(self, reference, width: int) -> ScoreBatch:
        """zsw_score_strands_batch_from: per read the better of sw_score_from_i{width} on the read and on its reverse complement
        (ties: forward); ScoreBatch.strand says which one answered."""
        torch = _torch()
        self._prep(reference)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        score = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status, tier, strand = (torch.empty(max(n, 1), dtype=torch.uint8, device=dev) for _ in range(3))
        b = self.reads.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_strands_batch_from(self.ctx.h, C.byref(b), width, self.preset, score.data_ptr(), status.data_ptr(),
                                                                 tier.data_ptr(), strand.data_ptr(), self.ctx.stream()))
        return ScoreBatch(score[:n], status[:n], tier=tier[:n], strand=strand[:n])

    def sw_score_strands_from_i8(self, reference) -> ScoreBatch:
        return self._score_strands_from(reference, 8)

    def sw_score_strands_from_i16(self, reference) -> ScoreBatch:
        return self._score_strands_from(reference, 16)

    def sw_score_strands_from_i32(self, reference) -> ScoreBatch:
        return self._score_strands_from(reference, 32)

    def _score_panel_from(self, width: int) -> ScoreBatch:
        """zsw_score_panel_batch_from: per read sw_score_from_i{width} against the member of the context's panel
        (`SwContext.set_panel`) that ranks highest, ties to the lowest member; ScoreBatch.ref says which one answered."""
        torch = _torch()
        self.ctx.set_scoring(self.matrix, self.gap_open, self.gap_extend)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        score, ref = (torch.empty(max(n, 1), dtype=torch.int32, device=dev) for _ in range(2))
        status, tier = (torch.empty(max(n, 1), dtype=torch.uint8, device=dev) for _ in range(2))
        b = self.reads.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_panel_batch_from(self.ctx.h, C.byref(b), width, self.preset, score.data_ptr(), status.data_ptr(),
                                                               tier.data_ptr(), ref.data_ptr(), self.ctx.stream()))
        return ScoreBatch(score[:n], status[:n], tier=tier[:n], ref=ref[:n])

    def sw_score_panel_from_i8(self) -> ScoreBatch:
        return self._score_panel_from(8)

    def sw_score_panel_from_i16(self) -> ScoreBatch:
        return self._score_panel_from(16)

    def sw_score_panel_from_i32(self) -> ScoreBatch:
        return self._score_panel_from(32)

    def sw_align_strands_from_i8_3pass(self, seq: SeqSrc) -> AlignmentBatch:
        """zsw_align_3pass_strands_batch_from: sw_align_from_i8_3pass of the read or of its reverse complement, whichever scores
        higher (ties: forward); AlignmentBatch.strand says which, and the coordinates are those of the sequence as aligned."""
        return self._align(seq, None, 8, self.preset, three_pass=True, strands=True)

    def sw_align_strands_from_i16_3pass(self, seq: SeqSrc) -> AlignmentBatch:
        return self._align(seq, None, 16, self.preset, three_pass=True, strands=True)

    def sw_align_strands_from_i32_3pass(self, seq: SeqSrc) -> AlignmentBatch:
        return self._align(seq, None, 32, self.preset, three_pass=True, strands=True)

    def _ranges_from(self, seq: SeqSrc, width: int) -> ScoreBatch:
        """profile_set.rs:313-362: sw_score_ranges over the tiers i{width} -> i32 of this preset"""
        torch = _torch()
        self._prep(seq.seq)
        n = self.reads.n_reads
        dev = self.reads.bases.device
        o = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for _ in range(5)]
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        tier = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = self.reads.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_ranges_batch_from(self.ctx.h, C.byref(b), width, self.preset, o[0].data_ptr(), o[1].data_ptr(),
                                                                o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), status.data_ptr(),
                                                                tier.data_ptr(), self.ctx.stream()))
        rs, re_, qs, qe = (x[:n] for x in o[1:])
        if seq.is_query:
            rs, re_, qs, qe = qs, qe, rs, re_
        return ScoreBatch(o[0][:n], status[:n], tier=tier[:n], ref_start=rs, ref_end=re_, query_start=qs, query_end=qe)

    def sw_score_ranges_from_i8(self, seq: SeqSrc) -> ScoreBatch:
        return self._ranges_from(seq, 8)

    def sw_score_ranges_from_i16(self, seq: SeqSrc) -> ScoreBatch:
        return self._ranges_from(seq, 16)

    def sw_score_ranges_from_i32(self, seq: SeqSrc) -> ScoreBatch:
        return self._ranges_from(seq, 32)

    def sw_align_from_i8(self, seq: SeqSrc) -> AlignmentBatch:
        return self._align(seq, None, 8, self.preset)

    def sw_align_from_i16(self, seq: SeqSrc) -> AlignmentBatch:
        return self._align(seq, None, 16, self.preset)

    def sw_align_from_i8_3pass(self, seq: SeqSrc) -> AlignmentBatch:
        """profile_set.rs:212-229 → sw_align_3pass (three_pass.rs:21-104)"""
        return self._align(seq, None, 8, self.preset, three_pass=True)

    def sw_align_from_i16_3pass(self, seq: SeqSrc) -> AlignmentBatch:
        return self._align(seq, None, 16, self.preset, three_pass=True)

    def sw_align_from_i32_3pass(self, seq: SeqSrc) -> AlignmentBatch:
        return self._align(seq, None, 32, self.preset, three_pass=True)

    def sw_align_from_i32(self, seq: SeqSrc) -> AlignmentBatch:
        return self._align(seq, None, 32, self.preset)


FILTER_REJECT, FILTER_PASS, FILTER_NONE = 0, 1, 2


def sneaky_snake(reference, reads, ref_start, ref_len, threshold: float, device: int = 0):
    """Batched `alignment::sneaky_snake(&reference[ref_start[i]..][..ref_len[i]], read_i, threshold)`
    (sneaky_snake.rs:78-131): a uint8 device tensor of FILTER_REJECT = Some(false) / FILTER_PASS = Some(true) /
    FILTER_NONE = None per read. `ref_start` / `ref_len`: one candidate window of `reference` per read."""
    torch = _torch()
    rb = _as_batch(reads, device)
    ctx = SwContext.get(rb.device_index)
    ctx.set_reference(reference)
    dev = rb.bases.device
    n = rb.n_reads
    rs = torch.as_tensor(np.asarray(ref_start, dtype=np.int64) if not isinstance(ref_start, torch.Tensor) else ref_start).to(dev, torch.int32).contiguous()
    rl = torch.as_tensor(np.asarray(ref_len, dtype=np.int64) if not isinstance(ref_len, torch.Tensor) else ref_len).to(dev, torch.int32).contiguous()
    if rs.numel() != n or rl.numel() != n:
        raise ValueError("one (ref_start, ref_len) window per read")
    out = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    b = rb.c_batch()
    ctx.check(ctx.lib.zsw_sneaky_snake_batch(ctx.h, C.byref(b), rs.data_ptr(), rl.data_ptr(), C.c_float(threshold), out.data_ptr(),
                                             ctx.stream()), profile_errors=False)
    return out[:n]


def into_local_profile(reads, matrix: WeightMatrix, gap_open: int, gap_extend: int, device: int = 0) -> LocalProfilesBatch:
    """Nucleotides::into_local_profile (nucleotides/mod.rs:262-266): the w256 preset."""
    return LocalProfilesBatch.new_with_w256(reads, matrix, gap_open, gap_extend, device)


class _SharedBase:
    """The one-profile-many-sequences role: the profile is built ONCE from `sequence` (sw/mod.rs:63-67 "the profile can be
    aligned against any number of different sequences") and every read of a batch is the sequence it is aligned against,
    walked row by row. Results follow the reference's conventions: `ref_*` is the non-profile sequence (the read) unless the
    reads are passed as `SeqSrc.Query(reads)`, which swaps the roles back (alignment/mod.rs:176-190)."""

    def __init__(self, sequence, matrix: WeightMatrix, gap_open: int, gap_extend: int, device: int = 0):
        if not isinstance(sequence, (bytes, bytearray, memoryview, np.ndarray)):
            # (this class once took the READS here; bytes(ReadBatch) or bytes(list) would be accepted and mean nothing)
            raise TypeError("the shared profile is built from ONE sequence (bytes); the reads are the arguments of its methods")
        sequence = bytes(sequence)
        validate_profile_args(len(sequence), gap_open, gap_extend)
        self.sequence = sequence
        self.matrix = matrix
        self.gap_open = gap_open
        self.gap_extend = gap_extend
        self.device = device
        self.ctx = SwContext.get(device)

    def _prep(self):
        self.ctx.set_scoring(self.matrix, self.gap_open, self.gap_extend)
        self.ctx.set_profile_sequence(self.sequence)

    @staticmethod
    def _reads_of(seq):
        """reads, or SeqSrc.Reference(reads) / SeqSrc.Query(reads) with a ReadBatch or a list of byte strings inside"""
        if isinstance(seq, SeqBatchSrc):
            return seq.reads, seq.is_query
        return seq, False

    def _ends(self, seq, direct) -> ScoreBatch:
        torch = _torch()
        reads, is_query = self._reads_of(seq)
        rb = _as_batch(reads, self.device)
        self._prep()
        n, dev = rb.n_reads, rb.bases.device
        score = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        rend = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        qend = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = rb.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_ends_shared_batch(self.ctx.h, C.byref(b), direct[0], direct[1], score.data_ptr(), rend.data_ptr(),
                                                                qend.data_ptr(), status.data_ptr(), self.ctx.stream()))
        if is_query:
            rend, qend = qend, rend
        return ScoreBatch(score[:n], status[:n], ref_end=rend[:n], query_end=qend[:n])

    def _ranges(self, seq, direct=None, from_width=None, preset=None) -> ScoreBatch:
        torch = _torch()
        reads, is_query = self._reads_of(seq)
        rb = _as_batch(reads, self.device)
        self._prep()
        n, dev = rb.n_reads, rb.bases.device
        o = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for _ in range(5)]
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        tier = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = rb.c_batch()
        if direct is not None:
            self.ctx.check(self.ctx.lib.zsw_score_ranges_shared_batch(self.ctx.h, C.byref(b), direct[0], direct[1], o[0].data_ptr(), o[1].data_ptr(),
                                                                      o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), status.data_ptr(),
                                                                      self.ctx.stream()))
        else:
            self.ctx.check(self.ctx.lib.zsw_score_ranges_shared_batch_from(self.ctx.h, C.byref(b), from_width, preset, o[0].data_ptr(), o[1].data_ptr(),
                                                                           o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), status.data_ptr(),
                                                                           tier.data_ptr(), self.ctx.stream()))
        rs, re_, qs, qe = (x[:n] for x in o[1:])
        if is_query:
            rs, re_, qs, qe = qs, qe, rs, re_
        return ScoreBatch(o[0][:n], status[:n], tier=tier[:n] if direct is None else None, ref_start=rs, ref_end=re_, query_start=qs, query_end=qe)

    def _align(self, seq, direct=None, from_width=None, preset=None, threepass=False) -> AlignmentBatch:
        torch = _torch()
        lib = self.ctx.lib
        f_direct = lib.zsw_align_3pass_shared_batch if threepass else lib.zsw_align_shared_batch
        f_from = lib.zsw_align_3pass_shared_batch_from if threepass else lib.zsw_align_shared_batch_from
        reads, is_query = self._reads_of(seq)
        rb = _as_batch(reads, self.device)
        self._prep()
        n, dev = rb.n_reads, rb.bases.device
        aln = torch.zeros(max(n, 1) * ALN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        tier = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        cap = max(8 * n, 64)
        b = rb.c_batch()
        total = C.c_uint64(0)
        while True:
            inc = torch.empty(cap, dtype=torch.int32, device=dev)
            op = torch.empty(cap, dtype=torch.uint8, device=dev)
            if direct is not None:
                rc = f_direct(self.ctx.h, C.byref(b), direct[0], direct[1], int(is_query), aln.data_ptr(), status.data_ptr(),
                              inc.data_ptr(), op.data_ptr(), cap, C.byref(total), self.ctx.stream())
            else:
                rc = f_from(self.ctx.h, C.byref(b), from_width, preset, int(is_query), aln.data_ptr(), status.data_ptr(),
                            tier.data_ptr(), inc.data_ptr(), op.data_ptr(), cap, C.byref(total), self.ctx.stream())
            if rc == -1 and total.value > cap:
                cap = int(total.value)
                continue
            self.ctx.check(rc)
            break
        torch.cuda.synchronize(dev)
        t = int(total.value)
        h_aln, h_status, h_inc, h_op, h_tier = _to_host(aln[: n * ALN_DTYPE.itemsize], status[:n], inc[:t], op[:t], tier[:n])
        return AlignmentBatch(h_status, h_aln.view(ALN_DTYPE), h_inc.view(np.uint32), h_op, h_tier if direct is None else None)


    def annotate(self, aln: AlignmentBatch, seq, residues: bool = False, verbose: bool = True):
        """zsw_annotate_batch over the alignments `aln` that one of this profile's alignment calls returned for `seq` (the same reads,
        or the same SeqBatchSrc); results as `_ProfileBatchBase.annotate`."""
        reads, is_query = self._reads_of(seq)
        rb = _as_batch(reads, self.device)
        self._prep()
        flags = _lib.ANNOTATE_SHARED | (0 if is_query else _lib.ANNOTATE_READ_IS_REF) | (_lib.ANNOTATE_MATCH_RESIDUES if residues else 0)
        return _annotate(self.ctx, rb, aln, flags, verbose)

    def pileup(self, aln: AlignmentBatch, seq, counts=None, insertions: bool = False):
        """zsw_pileup_batch over the alignments `aln` that one of this profile's alignment calls returned for `seq` (the same reads,
        or the same SeqBatchSrc): the table over the profile's own sequence; results as `_ProfileBatchBase.pileup`."""
        reads, is_query = self._reads_of(seq)
        rb = _as_batch(reads, self.device)
        self._prep()
        flags = _lib.ANNOTATE_SHARED | (0 if is_query else _lib.ANNOTATE_READ_IS_REF)
        return _pileup(self.ctx, rb, aln, flags, len(bytes(self.sequence)), counts, insertions)

    def to_sam_text(self, aln: AlignmentBatch, seq, qnames, quals=None, rname="ref", mapq: int = 255, strands=None, stats=None, omit_seq: bool = False,
                    device: bool = False):
        """zsw_sam_batch over the alignments `aln` that one of this profile's alignment calls returned for `seq` (the same reads, or
        the same SeqBatchSrc): as `_ProfileBatchBase.to_sam_text`, POS being the record's ref_start + 1 in whichever sequence the call
        gave the reference's role. The reads are taken as they are (no strand-aware call exists in this role)."""
        reads, _ = self._reads_of(seq)
        return _sam_text(self.ctx, _as_batch(reads, self.device), aln, qnames, quals, rname, mapq, strands, stats, omit_seq, device)


@dataclass
class SeqBatchSrc:
    """SeqSrc (alignment/mod.rs:161-166) over a batch of reads: which role the non-profile sequences play in the results."""

    reads: "object"
    is_query: bool

    @staticmethod
    def Reference(reads) -> "SeqBatchSrc":
        return SeqBatchSrc(reads, False)

    @staticmethod
    def Query(reads) -> "SeqBatchSrc":
        return SeqBatchSrc(reads, True)


class SharedStripedProfile(_SharedBase):
    """`StripedProfile::<T, N, S>::new(sequence, &matrix, gap_open, gap_extend)` once, used against every read of a batch
    (profile.rs:239-306, 440-552): sw_score(reads), sw_score_ends / sw_score_ranges / sw_align(SeqBatchSrc)."""

    def __init__(self, sequence, matrix: WeightMatrix, gap_open: int, gap_extend: int, T: str = "i16", N: int = 16, device: int = 0):
        if T not in _lib.INT_TYPES:
            raise ValueError(f"T must be one of {list(_lib.INT_TYPES)}")
        if T.startswith("u") and matrix.signed:
            raise ValueError("unsigned T needs matrix.to_biased_matrix() (profile.rs:215-219)")
        if T.startswith("i") and not matrix.signed:
            raise ValueError("signed T needs the signed matrix")
        super().__init__(sequence, matrix, gap_open, gap_extend, device)
        self.T, self.N = T, N

    def sw_score(self, reads) -> ScoreBatch:
        torch = _torch()
        rb = _as_batch(reads, self.device)
        self._prep()
        n, dev = rb.n_reads, rb.bases.device
        score = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = rb.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_shared_batch(self.ctx.h, C.byref(b), _lib.INT_TYPES[self.T], self.N, score.data_ptr(), status.data_ptr(),
                                                           self.ctx.stream()))
        return ScoreBatch(score[:n], status[:n])

    def sw_score_ends(self, seq) -> ScoreBatch:
        return self._ends(seq, (_lib.INT_TYPES[self.T], self.N))

    def sw_score_ranges(self, seq) -> ScoreBatch:
        return self._ranges(seq, direct=(_lib.INT_TYPES[self.T], self.N))

    def sw_align(self, seq) -> AlignmentBatch:
        return self._align(seq, direct=(_lib.INT_TYPES[self.T], self.N))

    def sw_align_3pass(self, seq) -> AlignmentBatch:
        """profile.rs:536-552 (three_pass.rs:21-104) with the shared profile: ranges, then banded / scalar alignment in the box"""
        return self._align(seq, direct=(_lib.INT_TYPES[self.T], self.N), threepass=True)


class SharedProfilesBatch(_SharedBase):
    """`SharedProfiles::new_with_w{128,256,512}(sequence, &matrix, gap_open, gap_extend)` (profile_set.rs:552-700) used against
    every read of a batch: the i8 -> i16 -> i32 cascade of `sw_score_from_i*`, `sw_score_ranges_from_i*`, `sw_align_from_i*`."""

    def __init__(self, sequence, matrix: WeightMatrix, gap_open: int, gap_extend: int, preset: int = 256, device: int = 0):
        if not matrix.signed:
            raise ValueError("profile sets take the signed matrix (profile_set.rs:552-560)")
        if preset not in (128, 256, 512):
            raise ValueError("preset must be 128, 256 or 512")
        super().__init__(sequence, matrix, gap_open, gap_extend, device)
        self.preset = preset

    @classmethod
    def new_with_w128(cls, sequence, matrix, gap_open, gap_extend, device=0):
        return cls(sequence, matrix, gap_open, gap_extend, 128, device)

    @classmethod
    def new_with_w256(cls, sequence, matrix, gap_open, gap_extend, device=0):
        return cls(sequence, matrix, gap_open, gap_extend, 256, device)

    @classmethod
    def new_with_w512(cls, sequence, matrix, gap_open, gap_extend, device=0):
        return cls(sequence, matrix, gap_open, gap_extend, 512, device)

    def _score_from(self, reads, width: int) -> ScoreBatch:
        torch = _torch()
        rb = _as_batch(reads, self.device)
        self._prep()
        n, dev = rb.n_reads, rb.bases.device
        score = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        tier = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b = rb.c_batch()
        self.ctx.check(self.ctx.lib.zsw_score_shared_batch_from(self.ctx.h, C.byref(b), width, self.preset, score.data_ptr(), status.data_ptr(),
                                                                tier.data_ptr(), self.ctx.stream()))
        return ScoreBatch(score[:n], status[:n], tier=tier[:n])

    def sw_score_from_i8(self, reads) -> ScoreBatch:
        return self._score_from(reads, 8)

    def sw_score_from_i16(self, reads) -> ScoreBatch:
        return self._score_from(reads, 16)

    def sw_score_from_i32(self, reads) -> ScoreBatch:
        return self._score_from(reads, 32)

    def sw_score_ranges_from_i8(self, seq) -> ScoreBatch:
        return self._ranges(seq, from_width=8, preset=self.preset)

    def sw_score_ranges_from_i16(self, seq) -> ScoreBatch:
        return self._ranges(seq, from_width=16, preset=self.preset)

    def sw_score_ranges_from_i32(self, seq) -> ScoreBatch:
        return self._ranges(seq, from_width=32, preset=self.preset)

    def sw_align_from_i8(self, seq) -> AlignmentBatch:
        return self._align(seq, from_width=8, preset=self.preset)

    def sw_align_from_i16(self, seq) -> AlignmentBatch:
        return self._align(seq, from_width=16, preset=self.preset)

    def sw_align_from_i32(self, seq) -> AlignmentBatch:
        return self._align(seq, from_width=32, preset=self.preset)

    def sw_align_from_i8_3pass(self, seq) -> AlignmentBatch:
        """ProfileSets::sw_align_from_i8_3pass (profile_set.rs:212-283) of SharedProfiles (:552-560)"""
        return self._align(seq, from_width=8, preset=self.preset, threepass=True)

    def sw_align_from_i16_3pass(self, seq) -> AlignmentBatch:
        return self._align(seq, from_width=16, preset=self.preset, threepass=True)

    def sw_align_from_i32_3pass(self, seq) -> AlignmentBatch:
        return self._align(seq, from_width=32, preset=self.preset, threepass=True)


def into_shared_profile(sequence, matrix: WeightMatrix, gap_open: int, gap_extend: int, device: int = 0) -> SharedProfilesBatch:
    """Nucleotides::into_shared_profile (nucleotides/mod.rs:295-299): SharedProfiles<32, 16, 8, S> of `sequence` (the w256 preset)"""
    return SharedProfilesBatch(sequence, matrix, gap_open, gap_extend, preset=256, device=device)
