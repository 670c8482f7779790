"""FASTQ ingest -> device read batches, and SAM emit: the data formats either side of the hot path.

Mirrors, for exactly what the path needs:
    FastQReader            src/data/records/fastq/reader.rs:17-187 (single-line FASTQ; same validation and messages)
    FastaReader            src/data/records/fasta/mod.rs:241-410 (multi-line FASTA; the same statements, checks and messages)
    SamData::from_alignment src/data/records/sam/mod.rs:223-245   (POS = ref_range.start + 1, CIGAR = states, AS:i = score;
                            with the stats of `annotate` also NM:i = mismatches + inserted + deleted bases)
    Display for SamData     src/data/records/sam/std_traits.rs:3-44 (tab-separated, optional fields appended)
    SAMReader               src/data/records/sam/reader.rs:189-286 (rows: a header line or a SamData; the same checks in the same order)
    SamData::is_unmapped / to_alignment   sam/mod.rs:305-354, over the two ciglet iterators of src/data/types/cigar/iter.rs:52-99, 478-537
                            and the merge of AlignmentStates::try_from (src/alignment/types/std_traits.rs:119-155)
    SamOptRaw::get          sam/mod.rs:517-540, 581-633 (the optional fields, parsed lazily)
"""
from __future__ import annotations

import io
import re
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


class FastaError(ValueError):
    """std::io::ErrorKind::InvalidData of the reference's FASTA reader; `code` is the ZSW_FASTA_* value of the failing check and `offset`
    where zsw_fasta_parse_batch points for it: the record's '>', or the first byte that is not whitespace for MISSING_GT."""

    def __init__(self, code: int, message: str, offset: int = 0):
        super().__init__(message)
        self.code, self.offset = code, offset


@dataclass
class Fasta:
    name: bytes  # the raw header bytes (the reference makes a String of them with from_utf8_lossy; nothing is an error)
    sequence: bytes


_ASCII_WHITESPACE = b" \t\n\x0c\r"  # u8::is_ascii_whitespace: no \x0b
_GT_HEADER = "FASTA records must start with the '>' symbol on a newline, and no other '>' symbols can occur in a header!"
_GT_SEQUENCE = "FASTA records must start with the '>' symbol on a newline, and no other '>' symbols can occur in a sequence!"


def _lines_ascii(b: bytes) -> List[bytes]:
    """SplitByByte2 over '\\n' and '\\r' (src/search/bytes/search.rs:23-79): nothing for an empty haystack, else one piece more than
    there are line-break bytes"""
    return re.split(b"[\n\r]", b) if b else []


class FastaReader:
    """Iterator over FASTA records (fasta/mod.rs:255-412), statement by statement: `read_first_record` for the file's first record,
    `next` for the others, both over `read_until`. `start` is the offset of the '>' of the record being read. continued: the stream
    starts at the '>' of a record that is not the file's first (what a caller that restarts at CONSUMED holds)."""

    def __init__(self, inner: BinaryIO, continued: bool = False):
        self._f = inner
        self._pending = b""
        self.offset = 0  # bytes read so far
        self.start = 0
        self.buffer = bytearray()
        self.first_record = True
        if continued:
            if self._read_until(b">", bytearray()) != 1:
                raise ValueError("a continued FASTA stream starts at '>'")
            self.first_record = False
            self.buffer = bytearray(b">")

    @staticmethod
    def from_readable(inner: BinaryIO) -> "FastaReader":
        buffered = inner if isinstance(inner, io.BufferedReader) else io.BufferedReader(inner)
        if not buffered.peek(1):
            raise FastaError(_lib.FASTA_NO_DATA, "No FASTA data was found!")
        return FastaReader(buffered)

    def _read_until(self, delim: bytes, buf: bytearray) -> int:
        """BufRead::read_until: appends up to and including `delim`, or to the end -> the bytes read"""
        n = 0
        while True:
            if not self._pending:
                self._pending = self._f.read(1 << 16)
                if not self._pending:
                    break
            i = self._pending.find(delim)
            take = len(self._pending) if i < 0 else i + 1
            buf += self._pending[:take]
            self._pending = self._pending[take:]
            n += take
            if i >= 0:
                break
        self.offset += n
        return n

    def __iter__(self) -> Iterator[Fasta]:
        return self

    def _error(self, code: int, msg: str, header: Optional[bytes] = None, offset: Optional[int] = None) -> FastaError:
        if header is not None:
            msg = f"{msg} See header: {header.decode('utf-8', 'replace')}"
        return FastaError(code, msg, self.start if offset is None else offset)

    def _read_first_record(self) -> Fasta:
        self.first_record = False
        while True:
            self.start = self.offset
            n = self._read_until(b"\n", self.buffer)
            if n == 0:
                self.buffer.clear()  # the iterator ends behind this error
                raise self._error(_lib.FASTA_NO_DATA, "No FASTA data found!", offset=0)
            if self.buffer.startswith(b">"):
                header = _chop_line_break(bytes(self.buffer[1:]))
                if not header:
                    raise self._error(_lib.FASTA_MISSING_HEADER, "Missing FASTA header!")
                if b">" in header:
                    raise self._error(_lib.FASTA_GT_IN_HEADER, _GT_HEADER, header)
                self.buffer.clear()
                self._read_until(b">", self.buffer)
                sequence = bytearray(b"".join(_lines_ascii(bytes(self.buffer))))
                if sequence.endswith(b">"):
                    sequence.pop()
                if not sequence:
                    raise self._error(_lib.FASTA_MISSING_SEQUENCE, "Missing FASTA sequence!", header)
                if not self.buffer.endswith(b"\n>"):
                    if self.buffer.endswith(b">"):
                        raise self._error(_lib.FASTA_GT_IN_SEQUENCE, _GT_SEQUENCE, header)
                    self.buffer.clear()
                return Fasta(header, bytes(sequence))
            elif all(c in _ASCII_WHITESPACE for c in self.buffer):
                self.buffer.clear()
            else:
                first = next(k for k, c in enumerate(self.buffer) if c not in _ASCII_WHITESPACE)
                raise self._error(_lib.FASTA_MISSING_GT, "The FASTA file must start with a '>' symbol!", offset=self.start + first)

    def __next__(self) -> Fasta:
        if self.first_record:
            return self._read_first_record()
        if not self.buffer:
            raise StopIteration
        self.start = self.offset - 1  # the '>' that ended the last read
        self.buffer.clear()
        self._read_until(b">", self.buffer)
        split = _lines_ascii(bytes(self.buffer))
        if not split:
            raise self._error(_lib.FASTA_MISSING_HEADER, "Missing FASTA header!")
        name = split[0]
        if not name:
            raise self._error(_lib.FASTA_MISSING_HEADER, "Missing FASTA header!")
        sequence = bytearray(b"".join(split[1:]))
        if sequence.endswith(b">"):
            sequence.pop()
        if not sequence:
            if self.buffer.endswith(b">"):
                if b"\n" in self.buffer:
                    raise self._error(_lib.FASTA_MISSING_SEQUENCE, "Missing FASTA sequence!", name)
                self._read_until(b"\n", self.buffer)
                raise self._error(_lib.FASTA_GT_IN_HEADER, _GT_HEADER, _chop_line_break(bytes(self.buffer)))
            raise self._error(_lib.FASTA_MISSING_SEQUENCE, "Missing FASTA sequence!", name)
        if not self.buffer.endswith(b"\n>"):
            if self.buffer.endswith(b">"):
                raise self._error(_lib.FASTA_GT_IN_SEQUENCE, _GT_SEQUENCE, name)
            self.buffer.clear()
        return Fasta(name, bytes(sequence))


def batch_from_fastq(records: List[FastQ], device: int = 0) -> ReadBatch:
    """Concatenates the sequences into one device-resident ragged (or fixed-length) batch."""
    return ReadBatch.from_sequences([r.sequence for r in records], device)


_U64 = (1 << 64) - 1
_CIGAR_OPS = b"MIDNSHPX="


class SamError(ValueError):
    """std::io::ErrorKind::InvalidData of the reference's SAM reader; `code` is the ZSW_SAMTEXT_* value of the failing check, `line`
    the index of the line among all lines and `offset` its first byte, where the reader knows them."""

    def __init__(self, code: int, message: str, line: Optional[int] = None, offset: Optional[int] = None):
        super().__init__(message)
        self.code, self.line, self.offset = code, line, offset


class SamOptError(ValueError):
    """the Err of SamOptRaw::get"""


class SamRecordError(ValueError):
    """the Err (or panic) of SamData::to_alignment; `code` is a ZSW_SAMREC_* value"""

    def __init__(self, code: int):
        super().__init__(f"SAM record cannot be converted (code {code})")
        self.code = code


@dataclass
class SamAlignment:
    """Alignment<u32> as to_alignment builds it; ciglets: (inc, op byte) with adjacent equal ops merged"""
    score: int
    ref_start: int
    ref_end: int
    query_start: int
    query_end: int
    ref_len: int
    query_len: int
    ciglets: list


def _rust_parse_int(s: str, lo: int, hi: int, signed: bool = False) -> int:
    """str::parse for an integer type with the range lo ..= hi: one optional '+' (for a signed type '+' or '-'), then at least one
    ASCII digit and nothing else; ValueError where it returns Err"""
    neg = False
    if s[:1] == "+" or (signed and s[:1] == "-"):
        neg = s[0] == "-"
        s = s[1:]
    if not s or any(c not in "0123456789" for c in s):
        raise ValueError("invalid digit found in string" if s else "cannot parse integer from empty string")
    v = -int(s) if neg else int(s)
    if not lo <= v <= hi:
        raise ValueError("number too large to fit in target type" if v > hi else "number too small to fit in target type")
    return v


def ciglets_unchecked(cigar: bytes):
    """CigletIterator (cigar/iter.rs:52-99): (inc, op) left to right; ends silently at a byte that is neither digit nor op, at an op
    without digits, at an inc beyond 64 bits and at the end (trailing digits are ignored); incs of 0 are yielded"""
    num, digits = 0, 0
    for b in cigar:
        if 48 <= b <= 57:
            num = num * 10 + (b - 48)
            digits += 1
            if num > _U64:
                return
        elif b in _CIGAR_OPS:
            if digits == 0:
                return
            yield num, b
            num, digits = 0, 0
        else:
            return


def ciglets_checked(cigar: bytes):
    """CigletIteratorChecked (cigar/iter.rs:478-537): (inc, op) left to right, SamRecordError at its first error"""
    num, digits = 0, 0
    for b in cigar:
        if 48 <= b <= 57:
            num = num * 10 + (b - 48)
            digits += 1
            if num > _U64:
                raise SamRecordError(_lib.SAMREC_CIGAR_INC_OVERFLOW)
        elif b in _CIGAR_OPS:
            if digits == 0:
                raise SamRecordError(_lib.SAMREC_CIGAR_MISSING_INC)
            if num == 0:
                raise SamRecordError(_lib.SAMREC_CIGAR_INC_ZERO)
            yield num, b
            num, digits = 0, 0
        else:
            raise SamRecordError(_lib.SAMREC_CIGAR_INVALID_OP)
    if digits:
        raise SamRecordError(_lib.SAMREC_CIGAR_MISSING_OP)


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

    def opt_get(self, tag: str):
        """SamOptRaw::get (sam/mod.rs:517-540): None, or (type character, value) of the first field with that tag — the value an int
        for type 'i', else the text as it stands; SamOptError where the reference returns Err."""
        for f in self.opt_fields:
            if ":" not in f:
                raise SamOptError(f"Invalid optional field {f}")
            this_tag, rest = f.split(":", 1)
            if this_tag != tag:
                continue
            if ":" not in rest:
                raise SamOptError(f"Invalid optional field {f}")
            type_text, value = rest.split(":", 1)
            tb = this_tag.encode("utf-8")
            if len(tb) != 2 or not (chr(tb[0]).isascii() and chr(tb[0]).isalpha()) or not (chr(tb[1]).isascii() and chr(tb[1]).isalnum()):
                raise SamOptError(f"Invalid SAM optional tag: {this_tag}")
            if len(type_text) != 1:
                raise SamOptError("Missing optional field type" if not type_text else f"Invalid optional field type {type_text}")
            if type_text == "i":
                try:
                    return "i", _rust_parse_int(value, -(1 << 63), (1 << 63) - 1, signed=True)
                except ValueError as e:
                    raise SamOptError(f"Failed to parse field '{f}' due to error: {e}") from e
            return type_text, value
        return None

    def score(self):
        """the AS tag as a score: opt_fields.get("AS") then .int(); None unless that is Ok(Some(v)) with 0 <= v <= 2^32 - 1"""
        try:
            got = self.opt_get("AS")
        except SamOptError:
            return None
        if got is None or got[0] != "i" or not 0 <= got[1] <= 0xFFFFFFFF:
            return None
        return got[1]

    def ref_len_in_alignment(self) -> int:
        """LenInAlignment over the unchecked CigletIterator (cigar/mod.rs:398-402), the sum saturating at 64 bits"""
        return min(sum(inc for inc, op in ciglets_unchecked(self.cigar.encode("utf-8")) if op in b"MDN=X"), _U64)

    def is_unmapped(self) -> bool:
        """sam/mod.rs:352-354"""
        return bool(self.flag & 4) or self.ref_len_in_alignment() == 0

    def to_alignment(self, score: int, ref_len: int):
        """sam/mod.rs:305-344 -> None (MaybeAligned::Unmapped) or a SamAlignment; where the reference returns Err or panics, or where
        a value leaves the 32-bit fields of zsw_alignment, SamRecordError with the first ZSW_SAMREC_* code in the order of
        include/zoe_sw.h (the reference may name the other fault of a record with two)."""
        if self.is_unmapped():
            return None
        cigar = self.cigar.encode("utf-8")
        if self.seq in (b"", b"*"):
            raise SamRecordError(_lib.SAMREC_SEQ_MISSING)
        raw = list(ciglets_checked(cigar))  # raises the first ciglet error
        merged: List[list] = []
        for inc, op in raw:
            if merged and merged[-1][1] == op:
                merged[-1][0] += inc
            else:
                merged.append([inc, op])
        if any(inc > _U64 for inc, _ in merged):
            raise SamRecordError(_lib.SAMREC_CIGAR_MERGE_OVERFLOW)
        if self.pos == 0:
            raise SamRecordError(_lib.SAMREC_POS_ZERO)
        rest = list(raw)  # next_ciglet_if_op / next_ciglet_back_if_op on the raw ciglets
        if rest and rest[0][1] == ord("H"):
            rest.pop(0)
        front = rest.pop(0)[0] if rest and rest[0][1] == ord("S") else 0
        if rest and rest[-1][1] == ord("H"):
            rest.pop()
        back = rest.pop()[0] if rest and rest[-1][1] == ord("S") else 0
        query_len = len(self.seq)
        if front + back > query_len:
            raise SamRecordError(_lib.SAMREC_CLIPS_EXCEED_SEQ)
        ref_start = self.pos - 1
        ref_end = min(ref_start + self.ref_len_in_alignment(), _U64)
        if any(inc > 0xFFFFFFFF for inc, _ in merged) or ref_end > 0xFFFFFFFF or query_len > 0xFFFFFFFF or len(merged) > 0xFFFFFFFF:
            raise SamRecordError(_lib.SAMREC_TOO_LARGE)
        return SamAlignment(score, ref_start, ref_end, front, front + (query_len - front - back), ref_len, query_len, [(i, o) for i, o in merged])

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


class SAMReader:
    """Iterator over the rows of SAM text (reader.rs:189-286): a `str` for a header line, a `SamData` for a data line, SamError where
    the reference's iterator yields Err. Lines are BufRead::lines': a line ends at "\n", which is removed with one "\r" in front of it.
    `line` counts the rows handed out so far and `offset` is the first byte of the next one."""

    def __init__(self, inner: BinaryIO):
        self._f = inner
        self.line = 0
        self.offset = 0

    @staticmethod
    def from_readable(inner: BinaryIO) -> "SAMReader":
        buffered = inner if isinstance(inner, io.BufferedReader) else io.BufferedReader(inner)
        if not buffered.peek(1):
            raise SamError(0, "No SAM data was found!")
        return SAMReader(buffered)

    def __iter__(self):
        return self

    def __next__(self):
        raw = self._f.readline()
        if not raw:
            raise StopIteration
        at, index = self.offset, self.line
        self.offset += len(raw)
        self.line += 1
        fail = lambda code, message: SamError(code, message, index, at)
        try:
            line = _chop_line_break(raw).decode("utf-8")
        except UnicodeDecodeError as e:
            raise fail(_lib.SAMTEXT_INVALID_UTF8, "stream did not contain valid UTF-8") from e
        if line.startswith("@"):
            return line
        parts = line.split("\t")
        if len(parts) < 11:
            raise fail(_lib.SAMTEXT_TOO_FEW_FIELDS, "SAM file did not have at least 11 fields!")
        try:
            flag = _rust_parse_int(parts[1], 0, 0xFFFF)
        except ValueError as e:
            raise fail(_lib.SAMTEXT_INVALID_FLAG, f"Error: {e}, invalid SAM bit flag '{parts[1]}'") from e
        try:
            pos = _rust_parse_int(parts[3], 0, _U64)
        except ValueError as e:
            raise fail(_lib.SAMTEXT_INVALID_POS, f"Error: {e}, invalid SAM reference position '{parts[3]}'") from e
        try:
            mapq = _rust_parse_int(parts[4], 0, 0xFF)
        except ValueError as e:
            raise fail(_lib.SAMTEXT_INVALID_MAPQ, f"Error: {e}, invalid SAM mapq '{parts[4]}'") from e
        cigar = parts[5].strip(" \t\n\x0c\r")  # trim_ascii
        if cigar == "*":
            cigar = ""
        qual = b"" if parts[10] in ("", "*") else parts[10].encode("utf-8")
        if any(c < 33 or c > 126 for c in qual):  # QualityScores: graphic ASCII
            raise fail(_lib.SAMTEXT_INVALID_QUALITY, "Invalid quality score byte!")
        return SamData(parts[0], flag, parts[2], pos, mapq, cigar, "*", 0, 0, parts[9].encode("utf-8"), qual, parts[11:])


class SamDeviceBatch:
    """What `sam_batch_from_text` returns: the data lines of SAM text as zsw_sam_parse_batch left them.

    reads          the device-resident `ReadBatch` (SEQ back to back with offsets): the reads AS ALIGNED, which is what `annotate` and
                   `pileup` of a profile batch over them walk
    quals          CUDA uint8, laid out as the reads' bases (forward: QUAL back to front where FLAG & 16)
    names          (CUDA uint8 names back to back, CUDA int64 n + 1 offsets): what `to_sam_text` takes as qnames
    alignments     the `AlignmentBatch` (host arrays, as `annotate`, `pileup` and `to_sam_text` take them). Its `.strand` is None: the
                   reads are oriented already, where the strand-aware alignment calls return alignments of reads still to be oriented
    strand         numpy uint8 per record: FLAG & 16. `to_sam_text` of a profile batch over `original_reads()` with `strands=.strand`
                   writes the lines back
    parsed         numpy, alignment.PARSED_DTYPE: pos, line, flag, mapq, code, bits per record
    report         the ZSW_SAMTEXT_INFO_* words; headers, consumed"""

    def __init__(self, reads: ReadBatch, quals, names, alignments: AlignmentBatch, strand, parsed, report):
        self.reads, self.quals, self.names, self.alignments, self.strand, self.parsed, self.report = reads, quals, names, alignments, strand, parsed, report
        self.consumed = int(report[_lib.SAMTEXT_INFO_CONSUMED])
        self.headers = int(report[_lib.SAMTEXT_INFO_HEADERS])

    def __len__(self) -> int:
        return self.reads.n_reads

    def original_reads(self) -> ReadBatch:
        """the reads as sequenced: those with FLAG & 16 reverse complemented back (zsw_orient_batch with the context's complement table)"""
        import torch

        from .alignment import SwContext

        if self.reads.n_reads == 0:
            return self.reads
        return SwContext.get(self.reads.device_index).orient(self.reads, torch.from_numpy(self.strand.copy()).to(self.reads.bases.device))


def sam_batch_from_text(text: bytes, rname=None, ref_len: int = 0, device: int = 0, final: bool = True, qual_forward: bool = True) -> SamDeviceBatch:
    """Uploads SAM text once and parses it on the device (zsw_sam_parse_batch): the records, reads, qualities and names ready for
    `annotate` / `pileup` / `to_sam_text` of a profile batch over `.reads`. rname: records of another RNAME are unmapped (the context
    has one reference); ref_len: the `ref_len` of every record. A malformed line raises SamError with the message SAMReader gives."""
    import numpy as np
    import torch

    from .alignment import ALN_DTYPE, PARSED_DTYPE, SwContext, _to_host

    ctx = SwContext.get(device)
    view = memoryview(text).cast("B")
    n = len(view)
    d_text = torch.frombuffer(bytearray(view) if n else bytearray(1), dtype=torch.uint8).to(torch.device("cuda", device))
    t, report = ctx.parse_sam(d_text, n, final=final, qual_forward=qual_forward, rname=rname, ref_len=ref_len)
    if report[_lib.SAMTEXT_INFO_ERROR]:
        at, line = int(report[_lib.SAMTEXT_INFO_ERROR_OFFSET]), int(report[_lib.SAMTEXT_INFO_ERROR_LINE])
        try:  # the reader's own message for that line
            next(SAMReader(io.BytesIO(bytes(view[at:]))))
        except SamError as e:
            raise SamError(e.code, f"line {line}: {e}", line, at) from None
        raise SamError(int(report[_lib.SAMTEXT_INFO_ERROR]), f"line {line} is malformed (code {int(report[_lib.SAMTEXT_INFO_ERROR])})", line, at)
    n_rec = int(report[_lib.SAMTEXT_INFO_RECORDS])
    aln, status, inc, op, strand, parsed = _to_host(t["aln"], t["status"], t["inc"], t["op"], t["strand"], t["parsed"])
    batch = AlignmentBatch(status.copy(), aln.view(ALN_DTYPE).copy(), inc.view(np.uint32).copy(), op.copy())
    reads = ReadBatch(t["bases"] if t["bases"].numel() else torch.zeros(1, dtype=torch.uint8, device=d_text.device), n_rec, offsets=t["offsets"],
                      min_len=int(report[_lib.SAMTEXT_INFO_MIN_LEN]) if n_rec else None)
    quals = t["quals"] if t["quals"].numel() else torch.zeros(1, dtype=torch.uint8, device=d_text.device)
    return SamDeviceBatch(reads, quals, (t["qnames"], t["qname_offsets"]), batch, strand.copy(), parsed.view(PARSED_DTYPE).copy(), report)


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


class FastaDeviceBatch:
    """What `fasta_batch_from_text` returns: the records of a FASTA buffer as zsw_fasta_parse_batch left them in device memory.

    bases          CUDA uint8, the sequences back to back (line breaks removed)
    offsets        CUDA int64, n + 1 entries
    names          CUDA uint8, the names back to back (raw header bytes)
    name_offsets   CUDA int64, n + 1 entries
    consumed       the offset one past the last record (a caller that reads a file in chunks restarts there, with continued=True)
    report         the ZSW_FASTA_INFO_* words"""

    def __init__(self, bases, offsets, names, name_offsets, report):
        self.bases, self.offsets, self.names, self.name_offsets, self.report = bases, offsets, names, name_offsets, report
        self.n_records = int(report[_lib.FASTA_INFO_RECORDS])
        self.consumed = int(report[_lib.FASTA_INFO_CONSUMED])
        self._host_offsets = None

    def __len__(self) -> int:
        return self.n_records

    def as_read_batch(self) -> ReadBatch:
        """the records as reads for the profile classes (there are no qualities: `to_sam_text` with quals=None prints '*')"""
        n = self.n_records
        return ReadBatch(self.bases, n, offsets=self.offsets, min_len=int(self.report[_lib.FASTA_INFO_MIN_LEN]) if n else None)

    def sequence(self, r: int):
        """record r's sequence as a view of the device array: what `SwContext.set_reference` takes without a copy"""
        if not 0 <= r < self.n_records:
            raise IndexError(f"record {r} of {self.n_records}")
        if self._host_offsets is None:
            self._host_offsets = self.offsets.cpu().numpy()
        return self.bases[int(self._host_offsets[r]):int(self._host_offsets[r + 1])]

    def records(self) -> List[Fasta]:
        """the `List[Fasta]` a FastaReader over the same bytes yields (with name_to_blank: `name` ends at the first blank)"""
        from .alignment import _to_host

        n = self.n_records
        if n == 0:
            return []
        bases, off, names, noff = _to_host(self.bases, self.offsets, self.names, self.name_offsets)
        b, nm = bases.tobytes(), names.tobytes()
        return [Fasta(nm[noff[i]:noff[i + 1]], b[off[i]:off[i + 1]]) for i in range(n)]


def fasta_batch_from_text(text: bytes, device: int = 0, final: bool = True, name_to_blank: bool = False, continued: bool = False) -> FastaDeviceBatch:
    """Uploads the bytes of a FASTA buffer once and parses them on the device (zsw_fasta_parse_batch, with the capacities that always
    suffice). final: the buffer ends the file; otherwise the record that starts at the buffer's last '>' is left, and `.consumed` is
    the offset of that '>'. continued: the buffer starts at the '>' of a record that is not the file's first. name_to_blank: names end
    in front of the first space or tab. A malformed text raises FastaError with the message FastaReader gives for it."""
    import ctypes as C

    import numpy as np
    import torch

    from .alignment import SwContext

    ctx = SwContext.get(device)
    dev = torch.device("cuda", device)
    view = memoryview(text).cast("B")
    n = len(view)
    d_text = torch.frombuffer(bytearray(view) if n else bytearray(1), dtype=torch.uint8).to(dev)
    base_cap, name_cap, record_cap = n, n, n // 4 + 1
    d_bases = torch.empty(max(base_cap, 1), dtype=torch.uint8, device=dev)
    d_names = torch.empty(max(name_cap, 1), dtype=torch.uint8, device=dev)
    d_off = torch.empty(record_cap + 1, dtype=torch.int64, device=dev)
    d_noff = torch.empty(record_cap + 1, dtype=torch.int64, device=dev)
    info = (C.c_uint64 * _lib.FASTA_INFO_WORDS)()
    flags = (_lib.FASTA_FINAL if final else 0) | (_lib.FASTA_NAME_TO_BLANK if name_to_blank else 0) | (_lib.FASTA_CONTINUED if continued else 0)
    ctx.check(ctx.lib.zsw_fasta_parse_batch(ctx.h, d_text.data_ptr(), n, _lib.MEM_DEVICE, flags, d_bases.data_ptr(), base_cap, d_off.data_ptr(), d_names.data_ptr(), name_cap,
                                            d_noff.data_ptr(), record_cap, info, ctx.stream()), profile_errors=False)
    report = np.array(list(info), dtype=np.uint64)
    code = int(report[_lib.FASTA_INFO_ERROR])
    if code:
        index = int(report[_lib.FASTA_INFO_ERROR_RECORD])
        try:  # the reader's own message: the records in front of the failing one are read again on the host
            for _ in FastaReader(io.BytesIO(bytes(view)), continued=continued):
                pass
        except FastaError as e:
            if e.code == code:
                raise FastaError(code, f"record {index}: {e}", int(report[_lib.FASTA_INFO_ERROR_OFFSET])) from None
        raise FastaError(code, f"FASTA record {index} is malformed (code {code})", int(report[_lib.FASTA_INFO_ERROR_OFFSET]))
    n_rec, n_bases, n_names = (int(report[k]) for k in (_lib.FASTA_INFO_RECORDS, _lib.FASTA_INFO_BASES, _lib.FASTA_INFO_NAME_BYTES))
    return FastaDeviceBatch(d_bases[:max(n_bases, 1)], d_off[:n_rec + 1], d_names[:max(n_names, 1)], d_noff[:n_rec + 1], report)


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
