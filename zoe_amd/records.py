"""FASTQ ingest -> device read batches, and SAM emit: the data formats either side of the hot path.

Mirrors, for exactly what the path needs:
    FastQReader            src/data/records/fastq/reader.rs:17-187 (single-line FASTQ; same validation and messages)
    SamData::from_alignment src/data/records/sam/mod.rs:223-245   (POS = ref_range.start + 1, CIGAR = states, AS:i = score;
                            with the stats of `annotate` also NM:i = mismatches + inserted + deleted bases)
    Display for SamData     src/data/records/sam/std_traits.rs:3-44 (tab-separated, optional fields appended)
"""
from __future__ import annotations

import io
from dataclasses import dataclass, field
from typing import BinaryIO, Iterator, List, Optional

from . import _lib
from .alignment import AlignmentBatch, ReadBatch, SOME


class FastQError(ValueError):
    """std::io::ErrorKind::InvalidData of the reference's reader."""


@dataclass
class FastQ:
    header: str
    sequence: bytes
    quality: bytes


def _chop_line_break(b: bytes) -> bytes:
    if b.endswith(b"\n"):
        b = b[:-1]
        if b.endswith(b"\r"):
            b = b[:-1]
    return b


class FastQReader:
    """Iterator over single-line FASTQ records (reader.rs:86-187)."""

    def __init__(self, inner: BinaryIO):
        self._f = inner

    @staticmethod
    def from_readable(inner: BinaryIO) -> "FastQReader":
        buffered = inner if isinstance(inner, io.BufferedReader) else io.BufferedReader(inner)
        if not buffered.peek(1):
            raise FastQError("No FASTQ data was found!")
        return FastQReader(buffered)

    @staticmethod
    def from_path(path) -> "FastQReader":
        try:
            f = open(path, "rb")
        except OSError as e:
            raise OSError(f"Failed to open path: {path}: {e}") from e
        try:
            return FastQReader.from_readable(f)
        except FastQError as e:
            raise FastQError(f"Failed to read data at path: {path}: {e}") from e

    def __iter__(self) -> Iterator[FastQ]:
        return self

    def __next__(self) -> FastQ:
        line = self._f.readline()
        if not line:
            raise StopIteration
        if not line.startswith(b"@"):
            raise FastQError("Missing '@' symbol at header line beginning! Ensure that the FASTQ file is not multi-line.")
        header = _chop_line_break(line[1:])
        if not header:
            raise FastQError("Missing FASTQ header!")
        try:
            header_s = header.decode("utf-8")
        except UnicodeDecodeError as e:
            raise FastQError(str(e)) from e
        seq = _chop_line_break(self._f.readline())
        if not seq:
            raise FastQError(f"Missing FASTQ sequence! See header: {header_s}")
        plus = self._f.readline()
        if not plus.startswith(b"+"):
            raise FastQError(f"Missing '+' line! Ensure that the FASTQ file is not multi-line. See header: {header_s}")
        qual = _chop_line_break(self._f.readline())
        if len(qual) != len(seq):
            if not qual:
                raise FastQError(f"Missing FASTQ quality scores! See header: {header_s}")
            raise FastQError(f"Sequence and quality score length mismatch ({len(seq)} ≠ {len(qual)})! See: {header_s}")
        if any(c < 33 or c > 126 for c in qual):  # QualityScores: graphic ASCII
            raise FastQError(f"Invalid quality score byte! See: {header_s}")
        return FastQ(header_s, seq, qual)


def batch_from_fastq(records: List[FastQ], device: int = 0) -> ReadBatch:
    """Concatenates the sequences into one device-resident ragged (or fixed-length) batch."""
    return ReadBatch.from_sequences([r.sequence for r in records], device)


@dataclass
class SamData:
    qname: str
    flag: int
    rname: str
    pos: int
    mapq: int
    cigar: str
    rnext: str = "*"
    pnext: int = 0
    tlen: int = 0
    seq: bytes = b"*"
    qual: bytes = b"*"
    opt_fields: List[str] = field(default_factory=list)

    @staticmethod
    def from_alignment(aln: AlignmentBatch, i: int, qname: str, flag: int, rname: str, mapq: int, seq: bytes, qual: bytes, stats=None) -> "SamData":
        """sam/mod.rs:223-245: both SAM and Alignment exclude clipped bases from positions; only the 1-based shift remains.
        stats: the stats array of `annotate` for this batch; appends NM:i:."""
        r = aln.records[i]
        opt = [f"AS:i:{int(r['score'])}"]
        if stats is not None:
            opt.append(f"NM:i:{int(AlignmentBatch.nm(stats[i:i + 1])[0])}")
        return SamData(qname, flag, rname, int(r["ref_start"]) + 1, mapq, aln.cigar(i), "*", 0, 0, seq, qual, opt)

    @staticmethod
    def unmapped(qname: str, seq: bytes, qual: bytes) -> "SamData":
        return SamData(qname, 4, "*", 0, 0, "*", "*", 0, 0, seq, qual, [])

    def __str__(self) -> str:
        seq = self.seq.decode() if self.seq else "*"
        qual = self.qual.decode() if self.qual else "*"
        core = f"{self.qname}\t{self.flag}\t{self.rname}\t{self.pos}\t{self.mapq}\t{self.cigar}\t{self.rnext}\t{self.pnext}\t{self.tlen}\t{seq}\t{qual}"
        return core + ("\t" + "\t".join(self.opt_fields) if self.opt_fields else "")


def align_fastq_to_sam(records: List[FastQ], reference: bytes, rname: str, matrix, gap_open: int, gap_extend: int,
                       device: int = 0, nm: bool = False, verbose_cigar: bool = False, three_pass: bool = False) -> List[SamData]:
    """FASTQ records -> `into_local_profile(..).sw_align_from_i8(SeqSrc::Reference(reference))` on the GPU -> SAM records
    (three_pass: `sw_align_from_i8_3pass`). nm: NM:i: on every mapped record; verbose_cigar: = / X in place of M — both from one
    `annotate` pass over the alignments."""
    from .alignment import SeqSrc, into_local_profile

    qnames = [r.header.split()[0] if r.header.split() else r.header for r in records]
    profiles = into_local_profile(batch_from_fastq(records, device), matrix, gap_open, gap_extend, device)
    src = SeqSrc.Reference(reference)
    aln = profiles.sw_align_from_i8_3pass(src) if three_pass else profiles.sw_align_from_i8(src)
    stats = None
    if nm or verbose_cigar:
        verbose, stats = profiles.annotate(aln, src, verbose=verbose_cigar)
        aln = verbose if verbose_cigar else aln
        stats = stats if nm else None
    out = []
    for i, r in enumerate(records):
        if int(aln.status[i]) == SOME:
            out.append(SamData.from_alignment(aln, i, qnames[i], 0, rname, 255, r.sequence, r.quality, stats))
        else:
            out.append(SamData.unmapped(qnames[i], r.sequence, r.quality))
    return out


def align_fastq_to_sam_text(records: List[FastQ], reference: bytes, rname: str, matrix, gap_open: int, gap_extend: int,
                            device: int = 0, nm: bool = False, verbose_cigar: bool = False, three_pass: bool = False) -> bytes:
    """The twin of `align_fastq_to_sam` that formats on the GPU (zsw_sam_batch): the same alignments, and the text
    `"\\n".join(str(r) for r in align_fastq_to_sam(..)) + "\\n"` as bytes, without a SamData per read on the host."""
    from .alignment import SeqSrc, into_local_profile

    if not records:
        return b""
    qnames = [r.header.split()[0] if r.header.split() else r.header for r in records]
    profiles = into_local_profile(batch_from_fastq(records, device), matrix, gap_open, gap_extend, device)
    src = SeqSrc.Reference(reference)
    aln = profiles.sw_align_from_i8_3pass(src) if three_pass else profiles.sw_align_from_i8(src)
    stats = None
    if nm or verbose_cigar:
        verbose, stats = profiles.annotate(aln, src, verbose=verbose_cigar)
        aln = verbose if verbose_cigar else aln
        stats = stats if nm else None
    return profiles.to_sam_text(aln, qnames, [r.quality for r in records], rname, 255, stats=stats)


class FastQDeviceBatch:
    """What `fastq_batch_from_text` returns: the records of a FASTQ buffer as zsw_fastq_parse_batch left them in device memory.

    reads          the device-resident `ReadBatch` (ragged: bases back to back with offsets; `min_len` as the report gives it)
    quals          CUDA uint8, laid out as the reads' bases
    names          CUDA uint8, the names back to back
    name_offsets   CUDA int64, n + 1 entries
    consumed       the offset one past the last record (a caller that reads a file in chunks restarts there)
    report         the ZSW_FASTQ_INFO_* words"""

    def __init__(self, reads: ReadBatch, quals, names, name_offsets, report):
        self.reads, self.quals, self.names, self.name_offsets, self.report = reads, quals, names, name_offsets, report
        self.consumed = int(report[_lib.FASTQ_INFO_CONSUMED])

    def __len__(self) -> int:
        return self.reads.n_reads

    def records(self) -> List[FastQ]:
        """the `List[FastQ]` a FastQReader over the same bytes yields (with name_to_blank: `header` is the name)"""
        from .alignment import _to_host

        n = self.reads.n_reads
        if n == 0:
            return []
        bases, quals, off, names, noff = _to_host(self.reads.bases, self.quals, self.reads.offsets, self.names, self.name_offsets)
        b, q, nm = bases.tobytes(), quals.tobytes(), names.tobytes()
        return [FastQ(nm[noff[i]:noff[i + 1]].decode("utf-8"), b[off[i]:off[i + 1]], q[off[i]:off[i + 1]]) for i in range(n)]


def fastq_batch_from_text(text: bytes, device: int = 0, final: bool = True, name_to_blank: bool = False) -> FastQDeviceBatch:
    """Uploads the bytes of a FASTQ buffer once and parses them on the device (zsw_fastq_parse_batch, with the capacities that always
    suffice). final: the buffer ends the file; otherwise only the records whose four lines are all terminated are parsed, and
    `.consumed` says where the rest begins. name_to_blank: names end in front of the first space or tab. A malformed record raises
    FastQError with the message FastQReader gives for it."""
    import ctypes as C

    import numpy as np
    import torch

    from .alignment import SwContext

    ctx = SwContext.get(device)
    dev = torch.device("cuda", device)
    view = memoryview(text).cast("B")
    n = len(view)
    d_text = torch.frombuffer(bytearray(view) if n else bytearray(1), dtype=torch.uint8).to(dev)
    base_cap, name_cap, record_cap = n // 2, n, n // 8 + 1
    d_bases = torch.empty(max(base_cap, 1), dtype=torch.uint8, device=dev)
    d_quals = torch.empty(max(base_cap, 1), dtype=torch.uint8, device=dev)
    d_names = torch.empty(max(name_cap, 1), dtype=torch.uint8, device=dev)
    d_off = torch.empty(record_cap + 1, dtype=torch.int64, device=dev)
    d_noff = torch.empty(record_cap + 1, dtype=torch.int64, device=dev)
    info = (C.c_uint64 * _lib.FASTQ_INFO_WORDS)()
    flags = (_lib.FASTQ_FINAL if final else 0) | (_lib.FASTQ_NAME_TO_BLANK if name_to_blank else 0)
    ctx.check(ctx.lib.zsw_fastq_parse_batch(ctx.h, d_text.data_ptr(), n, _lib.MEM_DEVICE, flags, d_bases.data_ptr(), d_quals.data_ptr(), base_cap, d_off.data_ptr(),
                                            d_names.data_ptr(), name_cap, d_noff.data_ptr(), record_cap, info, ctx.stream()), profile_errors=False)
    report = np.array(list(info), dtype=np.uint64)
    if report[_lib.FASTQ_INFO_ERROR]:
        at = int(report[_lib.FASTQ_INFO_ERROR_OFFSET])
        try:  # the reader's own message for that record
            next(FastQReader(io.BytesIO(bytes(view[at:]))))
        except FastQError:
            raise
        raise FastQError(f"FASTQ record {int(report[_lib.FASTQ_INFO_ERROR_RECORD])} is malformed (code {int(report[_lib.FASTQ_INFO_ERROR])})")
    n_rec, n_bases, n_names = (int(report[k]) for k in (_lib.FASTQ_INFO_RECORDS, _lib.FASTQ_INFO_BASES, _lib.FASTQ_INFO_NAME_BYTES))
    reads = ReadBatch(d_bases[:max(n_bases, 1)], n_rec, offsets=d_off[:n_rec + 1], min_len=int(report[_lib.FASTQ_INFO_MIN_LEN]) if n_rec else None)
    return FastQDeviceBatch(reads, d_quals[:max(n_bases, 1)], d_names[:max(n_names, 1)], d_noff[:n_rec + 1], report)


def align_fastq_text_to_sam_text(text: bytes, reference: bytes, rname: str, matrix, gap_open: int, gap_extend: int,
                                 device: int = 0, nm: bool = False, verbose_cigar: bool = False, three_pass: bool = False) -> bytes:
    """The twin of `align_fastq_to_sam_text` that starts from the bytes of a FASTQ file: parsed on the GPU (zsw_fastq_parse_batch,
    names up to the first space or tab), aligned, and formatted by zsw_sam_batch from the device arrays the parser wrote — names,
    bases and qualities never visit the host. A header that begins with a blank has an empty name here, where
    `align_fastq_to_sam_text` takes the first word behind it."""
    from .alignment import SeqSrc, into_local_profile

    fq = fastq_batch_from_text(text, device, final=True, name_to_blank=True)
    if len(fq) == 0:
        return b""
    profiles = into_local_profile(fq.reads, matrix, gap_open, gap_extend, device)
    src = SeqSrc.Reference(reference)
    aln = profiles.sw_align_from_i8_3pass(src) if three_pass else profiles.sw_align_from_i8(src)
    stats = None
    if nm or verbose_cigar:
        verbose, stats = profiles.annotate(aln, src, verbose=verbose_cigar)
        aln = verbose if verbose_cigar else aln
        stats = stats if nm else None
    return profiles.to_sam_text(aln, (fq.names, fq.name_offsets), fq.quals, rname, 255, stats=stats)
