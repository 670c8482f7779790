"""The case list of zsw_sam_parse_batch's tests, as byte strings, and what the call must give for each: the rows `records.SAMReader`
yields over the same bytes in front of its first SamError, converted by `SamData.is_unmapped` / `to_alignment` / `score`. Nothing
here knows the device's rules; the expectation is the mirror's own, and tests/test_records_sam.py pins the mirror by literals."""
import io

import numpy as np

from zoe_amd import _lib, records

FINAL, QUAL_FORWARD = 1, 2
FLAG_SETS = (FINAL, 0, FINAL | QUAL_FORWARD, QUAL_FORWARD)
INFO = ("records", "headers", "bases", "name_bytes", "ciglets", "consumed", "error", "error_line", "error_offset", "mapped", "coded", "min_len", "max_len")
SOME, UNMAPPED = 0, 2
(INVALID_UTF8, TOO_FEW_FIELDS, INVALID_FLAG, INVALID_POS, INVALID_MAPQ, INVALID_QUALITY) = range(1, 7)
(SEQ_MISSING, CIGAR_INVALID_OP, CIGAR_MISSING_INC, CIGAR_INC_ZERO, CIGAR_INC_OVERFLOW, CIGAR_MISSING_OP, CIGAR_MERGE_OVERFLOW, POS_ZERO, CLIPS_EXCEED_SEQ,
 TOO_LARGE) = range(1, 11)
BIT_NO_SCORE, BIT_OTHER_RNAME, BIT_SEQ_MISSING, BIT_QUAL_MISSING, BIT_QUAL_LENGTH = 1, 2, 4, 8, 16
U64 = (1 << 64) - 1


def parsed_part(text: bytes, final: bool) -> bytes:
    """the bytes a call looks at: all of them with FINAL, else the terminated lines"""
    return text if final else text[:text.rfind(b"\n") + 1]


class Expect:
    """what a call over `text` delivers; recs: per record a dict of name, bases, quals, status, aln (the nine zsw_alignment fields),
    ciglets [(inc, op)], strand, parsed (pos, line, flag, mapq, code, bits)"""

    def __init__(self, text: bytes, flags: int = FINAL, rname=None, ref_len: int = 0):
        part = parsed_part(text, bool(flags & FINAL))
        reader = records.SAMReader(io.BytesIO(part))
        self.recs, self.headers, self.error, self.message = [], 0, None, None
        n_cig = 0
        while True:
            at, line = reader.offset, reader.line
            try:
                row = next(reader)
            except StopIteration:
                break
            except records.SamError as e:
                assert (e.line, e.offset) == (line, at)
                self.error, self.message = e, str(e)
                break
            if isinstance(row, str):
                self.headers += 1
                continue
            bits, code, aln = 0, 0, None
            score = row.score()
            if score is None:
                bits |= BIT_NO_SCORE
            seq = b"" if row.seq in (b"", b"*") else row.seq
            if not seq:
                bits |= BIT_SEQ_MISSING
            if not row.qual:
                bits |= BIT_QUAL_MISSING
            elif len(row.qual) != len(seq):
                bits |= BIT_QUAL_LENGTH
            quals = b"!" * len(seq) if bits & (BIT_QUAL_MISSING | BIT_QUAL_LENGTH) else row.qual
            if (flags & QUAL_FORWARD) and (row.flag & 16):
                quals = quals[::-1]
            if not row.is_unmapped():
                if rname is not None and row.rname.encode("utf-8") != rname:
                    bits |= BIT_OTHER_RNAME
                else:
                    try:
                        aln = row.to_alignment(score or 0, ref_len)
                    except records.SamRecordError as e:
                        code = e.code
            ciglets = aln.ciglets if aln else []
            rec9 = (aln.score, aln.ref_start, aln.ref_end, aln.query_start, aln.query_end, aln.ref_len, aln.query_len, len(ciglets), n_cig) if aln else (0,) * 9
            n_cig += len(ciglets)
            self.recs.append(dict(name=row.qname.encode("utf-8"), bases=seq, quals=quals, status=SOME if aln else UNMAPPED, aln=rec9, ciglets=ciglets,
                                  strand=1 if row.flag & 16 else 0, parsed=(row.pos, line, row.flag, row.mapq, code, bits)))
        lens = [len(r["bases"]) for r in self.recs]
        e = self.error
        self.info = [len(self.recs), self.headers, sum(lens), sum(len(r["name"]) for r in self.recs), n_cig, e.offset if e else len(part), e.code if e else 0,
                     e.line if e else 0, e.offset if e else 0, sum(r["status"] == SOME for r in self.recs), sum(r["parsed"][4] != 0 for r in self.recs),
                     min(lens, default=0), max(lens, default=0)]

    def arrays(self):
        """the output arrays of a call that delivers these records, as numpy arrays / bytes"""
        r = self.recs
        from zoe_amd.alignment import ALN_DTYPE, PARSED_DTYPE

        return dict(
            bases=b"".join(x["bases"] for x in r), quals=b"".join(x["quals"] for x in r), qnames=b"".join(x["name"] for x in r),
            offsets=np.cumsum([0] + [len(x["bases"]) for x in r]).astype(np.uint64), qname_offsets=np.cumsum([0] + [len(x["name"]) for x in r]).astype(np.uint64),
            aln=np.array([x["aln"] for x in r], dtype=ALN_DTYPE) if r else np.zeros(0, dtype=ALN_DTYPE), status=np.array([x["status"] for x in r], dtype=np.uint8),
            inc=np.array([i for x in r for i, _ in x["ciglets"]], dtype=np.uint32), op=np.array([o for x in r for _, o in x["ciglets"]], dtype=np.uint8),
            strand=np.array([x["strand"] for x in r], dtype=np.uint8), parsed=np.array([x["parsed"] for x in r], dtype=PARSED_DTYPE) if r else np.zeros(0, dtype=PARSED_DTYPE))


def seq_of(n, k=0):
    return bytes(b"ACGTN"[(i * 7 + k) % 5] for i in range(n))


def qual_of(n, k=0):
    return bytes(33 + (i * 11 + k) % 94 for i in range(n))


def line(qname=b"q", flag=b"0", rname=b"chr", pos=b"1", mapq=b"255", cigar=b"4M", seq=b"ACGT", qual=None, opt=(b"AS:i:8",), eol=b"\n", mid=(b"*", b"0", b"0")):
    qual = qual_of(len(seq)) if qual is None else qual
    return b"\t".join((qname, flag, rname, pos, mapq, cigar) + tuple(mid) + (seq, qual) + tuple(opt)) + eol


def good(i: int) -> bytes:
    n = 10 + i
    return line(b"read%d" % i, b"16" if i & 1 else b"0", b"chr", b"%d" % (i + 1), b"%d" % (i * 50), b"%dM" % n, seq_of(n, i), qual_of(n, i), (b"AS:i:%d" % (2 * n),))


def five(bad: dict) -> bytes:
    """five lines, those of `bad` (index -> bytes) in place of the good ones"""
    return b"".join(bad.get(i, good(i)) for i in range(5))


FAULTS = {
    INVALID_UTF8: line(qname=b"q\x80"),
    TOO_FEW_FIELDS: b"q\t0\tchr\t1\t255\t4M\t*\t0\t0\tACGT\n",
    INVALID_FLAG: line(flag=b"65536"),
    INVALID_POS: line(pos=b"1x"),
    INVALID_MAPQ: line(mapq=b"256"),
    INVALID_QUALITY: line(qual=b"II I"),
}

INTEGERS = (b"+5", b"007", b"65535", b"65536", b"255", b"256", b"18446744073709551615", b"18446744073709551616", b"099999999999999999999", b"+", b"-0", b"", b"1 ", b" 1",
            b"1_0", b"0x1", b"-1", b"++1", b"00000000000000000000000000000000000004")
CIGARS = (b"0M", b"5I3Q", b"Q", b"*", b"4M", b"2S3S5M", b"3H2S5M2S3H", b"5S", b"3H", b"3M2M1I1I4M", b"18446744073709551615M1M", b"4294967296M", b"4294967295M",
          b"18446744073709551616M", b"4M3", b"M", b"4M0I", b"4Mx", b"4m", b" 4M ", b"\r4M\x0c", b"4M 2I", b"00000000000000000000004M", b"2S2M", b"1H1H4M",
          b"4M2S1S", b"9S4M", b"4M5S5S", b"2M2D2N2=2X2I2P", b"4M99999999999999999999999I", b"0M4M", b"4M5I3Q", b"4M18446744073709551615I1I", b"3Q0M")
SCORES = ((), (b"AS:i:-1",), (b"AS:f:1",), (b"AS:i:4294967296",), (b"AS:i:4294967295",), (b"XX", b"AS:i:5"), (b"AS:i:5", b"AS:i:6"), (b"AS:ii:3",), (b"NM:i:2", b"AS:i:9"),
          (b"AS:i:+7",), (b"AS:i:-0",), (b"AS:i:",), (b"AS:i",), (b"AS",), (b"AS:",), (b"AS::5",), (b"as:i:5",), (b"ASX:i:5",), (b"AS:i:5:6",), (b"AS:i: 5",),
          (b"AS:i:9223372036854775808",), (b"AS:i:-9223372036854775809",), (b"XS:Z:a:b", b"AS:i:3"), (b"MD:Z:" + b"10A" * 40, b"AS:i:77"), (b"",), (b"", b"AS:i:1"),
          ("AS:é:1".encode(),), (b"AS:Z:5",), (b"A:i:5", b"AS:i:4"))


def cases():
    c = []
    c.append(("empty", b""))
    c.append(("valid_lf", five({})))
    c.append(("valid_crlf", b"".join(good(i).replace(b"\n", b"\r\n") for i in range(5))))
    c.append(("valid_no_final_newline", five({})[:-1]))
    c.append(("valid_crlf_no_final_newline", good(0) + good(1)[:-1] + b"\r"))  # the bare '\r' stays: AS:i:22\r is no score
    c.append(("bare_cr_ends_qual", good(0) + line(opt=())[:-1] + b"\r"))        # ... and here it is a quality byte that is none
    c.append(("bare_cr_inside_a_line", line(qname=b"a\rb")))
    c.append(("cr_cr_lf", line(eol=b"\r\r\n")))
    c.append(("headers_on_top", b"@HD\tVN:1.6\n@SQ\tSN:chr\tLN:100\n" + five({})))
    c.append(("header_in_the_middle", good(0) + good(1) + b"@CO\tmiddle\n" + good(2) + b"@\n" + good(3)))
    c.append(("only_headers", b"@HD\n@SQ\n"))
    c.append(("only_a_header_unterminated", b"@HD"))
    c.append(("qname_with_at", good(0) + line(qname=b"@q") + good(1)))  # a header line by the reader's rule
    c.append(("blank_line", good(0) + b"\n" + good(1)))
    c.append(("blank_line_at_the_end", five({}) + b"\n"))
    c.append(("only_a_newline", b"\n"))
    c.append(("one_byte", b"A"))
    c.append(("header_not_utf8", good(0) + b"@CO\t\xff\n" + good(1)))
    for code, bad in FAULTS.items():
        for at in (0, 2, 4):
            c.append((f"code{code}_at{at}", five({at: bad})))
    c.append(("two_faults_flag_and_mapq", five({2: line(flag=b"x", mapq=b"300")})))
    c.append(("two_faults_utf8_and_fields", five({2: b"q\x80\t0\n"})))
    c.append(("two_faults_pos_and_quality", five({2: line(pos=b"", qual=b"\x7f\x7f\x7f\x7f")})))
    c.append(("two_bad_lines", five({3: FAULTS[INVALID_QUALITY], 1: FAULTS[INVALID_MAPQ]})))
    c.append(("two_bad_lines_late_first", five({4: FAULTS[TOO_FEW_FIELDS], 2: FAULTS[INVALID_POS]})))
    c.append(("ten_fields_trailing_tab", b"q\t0\tchr\t1\t255\t4M\t*\t0\t0\t\n"))
    c.append(("eleven_empty_fields", b"\t" * 10 + b"\n"))
    for k, v in enumerate(INTEGERS):
        c.append((f"flag_{k}", good(0) + line(flag=v)))
        c.append((f"pos_{k}", good(0) + line(pos=v)))
        c.append((f"mapq_{k}", good(0) + line(mapq=v)))
    for k, v in enumerate(CIGARS):
        c.append((f"cigar_{k}", line(cigar=v, seq=seq_of(12)) + good(1)))
    c.append(("flag4_good_cigar", line(flag=b"4")))
    c.append(("flag4_everything_else_bad", line(flag=b"20", pos=b"0", cigar=b"4Q", seq=b"*")))
    for k, v in enumerate(SCORES):
        c.append((f"score_{k}", line(opt=v) + good(1)))
    c.append(("seq_missing_star", line(seq=b"*", qual=b"*")))
    c.append(("seq_missing_empty", line(seq=b"", qual=b"")))
    c.append(("seq_missing_qual_present", line(seq=b"*", qual=b"IIII")))
    c.append(("seq_missing_and_cigar_bad", line(seq=b"*", cigar=b"4M3")))
    c.append(("cigar_bad_and_pos_zero", line(cigar=b"4M0I", pos=b"0")))
    c.append(("merge_overflow_and_later_op_error", line(cigar=b"18446744073709551615M1M4Q")))
    c.append(("pos_zero", line(pos=b"0")))
    c.append(("pos_zero_and_clips", line(pos=b"0", cigar=b"9S4M")))
    c.append(("clips_and_too_large", line(cigar=b"9S4294967296M")))
    c.append(("ref_end_too_large", line(pos=b"4294967293", cigar=b"4M")))
    c.append(("ref_end_just_fits", line(pos=b"4294967292", cigar=b"4M")))
    c.append(("pos_huge", line(pos=b"18446744073709551615", cigar=b"4M")))
    c.append(("qual_missing", line(qual=b"*") + line(qual=b"")))
    c.append(("qual_other_length", line(qual=b"III") + line(qual=b"IIIII")))
    c.append(("qual_on_flag16", line(flag=b"16", qual=b"!#%'") + line(flag=b"16", qual=b"*") + line(flag=b"0", qual=b"!#%'")))
    c.append(("other_rname", line(rname=b"chr") + line(rname=b"chr2") + line(rname=b"ch") + line(rname=b"chR") + line(rname=b"*", flag=b"4") + line(rname=b"other", cigar=b"4Q")))
    c.append(("long_rname", line(rname=b"r" * 130) + line(rname=b"r" * 129 + b"x")))
    c.append(("mid_fields_ignored", line(mid=(b"\xc3\xa9", b"x", b"-"))))
    edge = (0, 1, 63, 64, 65, 127, 128, 129)
    c.append(("qname_lengths", b"".join(line(qname=b"n" * n) for n in edge)))
    c.append(("rname_lengths", b"".join(line(rname=b"c" * n) for n in edge)))
    c.append(("seq_lengths", b"".join(line(qname=b"s%d" % n, cigar=b"%dM" % n, seq=seq_of(n, n), qual=qual_of(n, n)) for n in (1, 63, 64, 65, 1000))))
    c.append(("number_lengths", b"".join(line(flag=b"0" * (n - 1) + b"3", pos=b"0" * (n - 1) + b"7", mapq=b"0" * (n - 1) + b"9") for n in edge[1:])))
    # CIGARs of 0 .. 129 bytes: every sweep boundary inside a number and on an op
    for n in edge:
        body = b"".join(b"%d%s" % (1 + k % 9, b"MI"[k % 2:k % 2 + 1]) for k in range(n // 2))
        cig = (b"0" * (n - len(body)) + body)[:n] if n else b""
        c.append((f"cigar_len_{n}", line(cigar=cig, seq=seq_of(400)) + line(cigar=cig[1:] + b"M", seq=seq_of(400))))
    c.append(("cigar_number_across_sweep", line(cigar=b"1M" * 31 + b"12345M", seq=seq_of(30))))
    c.append(("cigar_run_across_sweep", line(cigar=b"1M" * 40 + b"2I" + b"1M" * 40, seq=seq_of(82))))
    c.append(("opt_lengths", b"".join(line(opt=(b"XA:Z:" + b"z" * n, b"AS:i:%d" % n)) for n in edge)))
    return c


CASES = cases()


def mixed_file(n, seed=1, max_read=400, max_ciglets=40, rnames=(b"chr",)):
    """n lines: mapped and unmapped, headers interleaved, CIGARs of 1 .. max_ciglets ciglets, reads of 1 .. max_read bases"""
    rng = np.random.default_rng(seed)
    out = [b"@HD\tVN:1.6\n"]
    for i in range(n):
        kind = int(rng.integers(0, 20))
        if kind == 0:
            out.append(b"@CO\tline %d\n" % i)
            continue
        L = int(rng.integers(1, max_read + 1)) if i > 1 else (1, max_read)[i]
        k = min(int(rng.integers(1, max_ciglets + 1)), L)
        cuts = np.sort(rng.choice(np.arange(1, L), size=k - 1, replace=False)) if k > 1 else np.zeros(0, dtype=np.int64)
        parts = np.diff(np.concatenate(([0], cuts, [L])))
        ops = [b"MI"[j % 2:j % 2 + 1] for j in range(k)]
        cigar = b"".join(b"%d%s" % (int(p), o) for p, o in zip(parts, ops))
        flag = (16 if rng.integers(0, 2) else 0) | (4 if kind == 1 else 0)
        rn = rnames[int(rng.integers(0, len(rnames)))]
        out.append(line(b"read_%d" % i, b"%d" % flag, rn, b"%d" % int(rng.integers(1, 1000)), b"%d" % int(rng.integers(0, 256)), b"*" if kind == 2 else cigar,
                        seq_of(L, i), qual_of(L, i) if kind != 3 else b"*", (b"AS:i:%d" % L, b"NM:i:0") if kind != 4 else ()))
    return b"".join(out)
