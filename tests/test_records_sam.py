"""The mirror of the reference's SAM reader in zoe_amd/records.py (SAMReader, SamData.is_unmapped / to_alignment / opt_get / score),
pinned by literal expectations derived by hand from the reference's lines (src/data/records/sam/reader.rs:189-286, sam/mod.rs:305-354,
517-540, 581-633, src/data/types/cigar/iter.rs:52-99, 478-537, src/alignment/types/std_traits.rs:119-155) — not produced by the mirror
— and the round trip on the CPU: tests/sam_ref.py's lines over oracle alignments of both strands, back through the mirror."""
import io
import re

import numpy as np
import pytest

import sam_ref
import samtext_cases as sc
from zoe_amd import records
from zoe_amd.records import SamAlignment, SamData, SamError, SamRecordError, SAMReader

M, I, D, S, H = (ord(c) for c in "MIDSH")


def rows(text: bytes):
    return list(SAMReader(io.BytesIO(text)))


def reader_error(text: bytes):
    """-> (rows delivered in front of the error, code, line, offset)"""
    r = SAMReader(io.BytesIO(text))
    n = 0
    with pytest.raises(SamError) as e:
        for _ in r:
            n += 1
    return n, e.value.code, e.value.line, e.value.offset


def convert(**kw):
    """one line through the reader and to_alignment -> "unmapped", a ZSW_SAMREC_* code, or the SamAlignment"""
    (row,) = rows(sc.line(**kw))
    try:
        a = row.to_alignment(row.score() or 0, 1000)
    except SamRecordError as e:
        return e.code
    return "unmapped" if a is None else a


def test_every_reader_code_at_the_first_a_middle_and_the_last_line():
    lens = [len(sc.good(i)) for i in range(5)]
    for code, bad in sc.FAULTS.items():
        for at in (0, 2, 4):
            assert reader_error(sc.five({at: bad})) == (at, code, at, sum(lens[:at])), (code, at)
    assert (sc.INVALID_UTF8, sc.TOO_FEW_FIELDS, sc.INVALID_FLAG, sc.INVALID_POS, sc.INVALID_MAPQ, sc.INVALID_QUALITY) == (1, 2, 3, 4, 5, 6)
    assert len(rows(sc.five({}))) == 5


def test_the_earlier_check_wins_on_a_line_and_the_lower_line_wins_in_a_file():
    assert reader_error(sc.line(flag=b"x", mapq=b"300"))[1] == 3               # FLAG is parsed before MAPQ
    assert reader_error(b"q\x80\t0\n")[1] == 1                                  # lines() fails before the fields are counted
    assert reader_error(sc.line(pos=b"", qual=b"\x7f\x7f\x7f\x7f"))[1] == 4    # POS before QUAL
    assert reader_error(sc.line(mapq=b"-1", qual=b" "))[1] == 5
    assert reader_error(b"q\t0\tchr\tx\n")[1] == 2                              # the count comes before any field
    assert reader_error(sc.five({3: sc.FAULTS[6], 1: sc.FAULTS[5]}))[:3] == (1, 5, 1)
    assert reader_error(sc.five({4: sc.FAULTS[2], 2: sc.FAULTS[4]}))[:3] == (2, 4, 2)


@pytest.mark.parametrize("field, bits", [("flag", 16), ("pos", 64), ("mapq", 8)])
def test_the_integer_parser(field, bits):
    top = (1 << bits) - 1
    good = {b"+5": 5, b"007": 7, b"0": 0, b"+0": 0, b"%d" % top: top, b"0%d" % top: top, b"+%d" % top: top, b"0" * 40 + b"9": 9}
    bad = [b"%d" % (top + 1), b"+", b"-", b"-0", b"-1", b"", b"1 ", b" 1", b"1_0", b"0x1", b"++1", b"1+", b"1.0", "１".encode(), b"9" * 21]
    for text, want in good.items():
        (row,) = rows(sc.line(**{field: text}))
        assert getattr(row, field) == want, text
    for text in bad:
        assert reader_error(sc.line(**{field: text}))[1] == {"flag": 3, "pos": 4, "mapq": 5}[field], text
    if field == "flag":
        assert rows(sc.line(flag=b"65535"))[0].flag == 65535 and reader_error(sc.line(flag=b"65536"))[1] == 3
    if field == "mapq":
        assert rows(sc.line(mapq=b"255"))[0].mapq == 255 and reader_error(sc.line(mapq=b"256"))[1] == 5
    if field == "pos":  # 20 digits: the largest usize; 21 digits: a leading zero is fine, a value beyond 64 bits is not
        assert rows(sc.line(pos=b"18446744073709551615"))[0].pos == 18446744073709551615
        assert rows(sc.line(pos=b"018446744073709551615"))[0].pos == 18446744073709551615
        assert reader_error(sc.line(pos=b"18446744073709551616"))[1] == 4 and reader_error(sc.line(pos=b"100000000000000000000"))[1] == 4


def test_lines_headers_and_line_breaks():
    g = [sc.good(i) for i in range(4)]
    got = rows(b"@HD\tVN:1.6\n" + g[0] + b"@CO\tin the middle\n" + g[1] + b"@\n")
    assert [type(r) for r in got] == [str, SamData, str, SamData, str] and got[0] == "@HD\tVN:1.6" and got[4] == "@"
    assert rows(sc.line(qname=b"@q")) == [sc.line(qname=b"@q")[:-1].decode()]  # a QNAME that begins with '@' makes a header line
    assert reader_error(g[0] + b"\n" + g[1]) == (1, 2, 1, len(g[0]))            # a blank line: one field
    assert reader_error(b"\n")[1:] == (2, 0, 0)
    crlf = rows(g[0].replace(b"\n", b"\r\n") + g[1].replace(b"\n", b"\r\n"))
    assert [r.opt_fields for r in crlf] == [["AS:i:20"], ["AS:i:22"]]
    assert rows(g[0] + g[1][:-1])[1].opt_fields == ["AS:i:22"]                  # no final newline
    assert rows(g[0] + g[1][:-1] + b"\r")[1].opt_fields == ["AS:i:22\r"]        # a bare '\r' stays
    assert reader_error(sc.line(opt=())[:-1] + b"\r")[1] == 6                   # ... where it ends QUAL it is no quality
    assert rows(sc.line(eol=b"\r\r\n"))[0].opt_fields == ["AS:i:8\r"]           # one '\r' is removed
    assert rows(b"") == []
    assert reader_error(g[0] + b"@CO\t\xff\n" + g[1])[:3] == (1, 1, 1)          # header lines are UTF-8 too
    assert rows(sc.line(mid=(b"\xc3\xa9", b"x", b"-")))[0].cigar == "4M"        # RNEXT, PNEXT, TLEN are not looked at
    with pytest.raises(SamError, match="No SAM data"):
        SAMReader.from_readable(io.BytesIO(b""))


def test_trim_ascii_on_the_cigar_and_the_star():
    assert rows(sc.line(cigar=b" 4M "))[0].cigar == "4M" and rows(sc.line(cigar=b"\r4M\x0c"))[0].cigar == "4M"
    assert rows(sc.line(cigar=b"4M 2I"))[0].cigar == "4M 2I"      # only the ends
    assert rows(sc.line(cigar=b"\x0b4M"))[0].cigar == "\x0b4M"    # a vertical tab is no ASCII whitespace to trim_ascii
    assert rows(sc.line(cigar=b"*"))[0].cigar == "" and rows(sc.line(cigar=b" * "))[0].cigar == ""
    assert convert(cigar=b" 4M ") == SamAlignment(8, 0, 4, 0, 4, 1000, 4, [(4, M)])
    assert convert(cigar=b"4M 2I") == 2 and convert(cigar=b"\x0b4M") == "unmapped"


def test_is_unmapped():
    for cigar in (b"0M", b"5I3Q", b"Q", b"*", b"", b"5S", b"3H", b"4I", b"M", b"x4M", b"18446744073709551616M", b"0M0D0N0=0X", b"3Q4M", b"I4M"):
        assert convert(cigar=cigar) == "unmapped", cigar
    assert convert(flag=b"4") == "unmapped" and convert(flag=b"20", cigar=b"4Q", pos=b"0", seq=b"*") == "unmapped"
    # the unchecked iterator yields what lies in front of its stop, and incs of 0
    for cigar, ref in ((b"4M5I3Q", 4), (b"0M4M", 4), (b"2M2D2N2=2X2I2P", 10), (b"4M3", 4), (b"4MM", 4), (b"4M18446744073709551616D", 4)):
        (row,) = rows(sc.line(cigar=cigar))
        assert row.ref_len_in_alignment() == ref and not row.is_unmapped(), cigar


def test_every_conversion_code_and_the_winner_of_two_faults():
    assert convert(seq=b"*", qual=b"*") == 1 and convert(seq=b"", qual=b"") == 1
    assert convert(cigar=b"4M3Q") == 2 and convert(cigar=b"4Mx") == 2 and convert(cigar=b"4M2m") == 2
    assert convert(cigar=b"4MM") == 3 and convert(cigar=b"4MI2D") == 3
    assert convert(cigar=b"4M0I") == 4 and convert(cigar=b"0M4M") == 4
    assert convert(cigar=b"4M18446744073709551616I") == 5 and convert(cigar=b"4M99999999999999999999999") == 5
    assert convert(cigar=b"4M3") == 6 and convert(cigar=b"4M18446744073709551615") == 6
    assert convert(cigar=b"18446744073709551615M1M") == 7 and convert(cigar=b"4M18446744073709551615I1I") == 7
    assert convert(pos=b"0") == 8
    assert convert(cigar=b"9S4M") == 9 and convert(cigar=b"2S4M3S") == 9 and convert(cigar=b"4M", seq=b"A") == SamAlignment(8, 0, 4, 0, 1, 1000, 1, [(4, M)])
    assert convert(cigar=b"4294967296M") == 10 and convert(cigar=b"4294967295M1M") == 10 and convert(pos=b"4294967293") == 10
    assert convert(pos=b"4294967292") == SamAlignment(8, 4294967291, 4294967295, 0, 4, 1000, 4, [(4, M)])
    assert convert(pos=b"18446744073709551615") == 10 and convert(cigar=b"18446744073709551615M") == 10
    assert convert(cigar=b"4294967295M") == SamAlignment(8, 0, 4294967295, 0, 4, 1000, 4, [(4294967295, M)])
    # two faults: the order of the header, which is the lower code
    assert convert(seq=b"*", cigar=b"4M3") == 1
    assert convert(cigar=b"4M0I", pos=b"0") == 4
    assert convert(cigar=b"18446744073709551615M1M4Q") == 2   # a ciglet error anywhere comes before the merge
    assert convert(cigar=b"4Mx0I") == 2 and convert(cigar=b"4M0Ix") == 4 and convert(cigar=b"4M" + b"9" * 20 + b"x") == 5  # the first in the text
    assert convert(pos=b"0", cigar=b"9S4M") == 8
    assert convert(cigar=b"9S4294967296M") == 9
    assert convert(pos=b"0", cigar=b"18446744073709551615M1M") == 7


def test_clips_and_merging():
    seq = sc.seq_of(12)
    assert convert(cigar=b"2S3S5M", seq=seq) == SamAlignment(8, 0, 5, 2, 12, 1000, 12, [(5, S), (5, M)])
    assert convert(cigar=b"3H2S5M2S3H", seq=seq) == SamAlignment(8, 0, 5, 2, 10, 1000, 12, [(3, H), (2, S), (5, M), (2, S), (3, H)])
    assert convert(cigar=b"5S", seq=seq) == "unmapped" and convert(cigar=b"3H", seq=seq) == "unmapped"
    assert convert(cigar=b"4M2S1S", seq=seq) == SamAlignment(8, 0, 4, 0, 11, 1000, 12, [(4, M), (3, S)])
    assert convert(cigar=b"1H1H4M", seq=seq) == SamAlignment(8, 0, 4, 0, 12, 1000, 12, [(2, H), (4, M)])
    assert convert(cigar=b"2S4M", seq=seq) == SamAlignment(8, 0, 4, 2, 12, 1000, 12, [(2, S), (4, M)])
    assert convert(cigar=b"4M3S", seq=seq) == SamAlignment(8, 0, 4, 0, 9, 1000, 12, [(4, M), (3, S)])
    assert convert(cigar=b"2S1H4M", seq=seq) == SamAlignment(8, 0, 4, 2, 12, 1000, 12, [(2, S), (1, H), (4, M)])  # S then H: the H is not skipped
    assert convert(cigar=b"1S", seq=seq) == "unmapped"
    assert convert(cigar=b"4M1S", seq=seq, pos=b"7") == SamAlignment(8, 6, 10, 0, 11, 1000, 12, [(4, M), (1, S)])
    assert convert(cigar=b"3S4M", seq=seq).query_start == 3
    # one S between the ends is taken once: from the front
    assert convert(cigar=b"3S", seq=seq) == "unmapped"
    assert convert(cigar=b"3M2M1I1I4M", seq=seq) == SamAlignment(8, 0, 9, 0, 12, 1000, 12, [(5, M), (2, I), (4, M)])
    assert convert(cigar=b"2M2D2N2=2X2I2P", seq=seq).ciglets == [(2, M), (2, D), (2, ord("N")), (2, ord("=")), (2, ord("X")), (2, I), (2, ord("P"))]
    assert convert(cigar=b"00000000000000000000004M", seq=seq) == SamAlignment(8, 0, 4, 0, 12, 1000, 12, [(4, M)])


def test_the_score_is_what_get_as_then_int_gives():
    score = lambda *opt: rows(sc.line(opt=opt))[0].score()
    assert score() is None and score(b"NM:i:2") is None
    assert score(b"AS:i:8") == 8 and score(b"NM:i:2", b"AS:i:9") == 9 and score(b"AS:i:+7") == 7 and score(b"AS:i:-0") == 0 and score(b"AS:i:007") == 7
    assert score(b"AS:i:4294967295") == 4294967295 and score(b"AS:i:4294967296") is None and score(b"AS:i:-1") is None
    assert score(b"AS:f:1") is None and score(b"AS:Z:5") is None and score(b"AS:ii:3") is None and score(b"AS::5") is None and score("AS:é:1".encode()) is None
    assert score(b"XX", b"AS:i:5") is None          # a field without a colon in front of AS: Err
    assert score(b"AS:i:5", b"XX") == 5             # ... behind it: never looked at
    assert score(b"AS:i:5", b"AS:i:6") == 5 and score(b"AS:f:5", b"AS:i:6") is None  # the first AS decides
    assert score(b"AS:i:") is None and score(b"AS:i") is None and score(b"AS") is None and score(b"AS:") is None and score(b"AS:i: 5") is None
    assert score(b"AS:i:5:6") is None and score(b"as:i:5") is None and score(b"ASX:i:5") is None and score(b"A:i:5", b"AS:i:4") == 4
    assert score(b"XS:Z:a:b", b"AS:i:3") == 3 and score(b"", b"AS:i:1") is None and score(b"AS:i:9223372036854775808") is None
    row = rows(sc.line(opt=(b"XS:Z:a:b", b"NM:i:-3", b"AS:A:x")))[0]
    assert row.opt_get("XS") == ("Z", "a:b") and row.opt_get("NM") == ("i", -3) and row.opt_get("AS") == ("A", "x") and row.opt_get("ZZ") is None
    with pytest.raises(records.SamOptError):
        rows(sc.line(opt=(b"N1:i:x",)))[0].opt_get("N1")
    with pytest.raises(records.SamOptError):
        rows(sc.line(opt=(b"1N:i:1",)))[0].opt_get("1N")  # parse_tag: the first byte a letter


def test_qual_missing_of_another_length_and_forward():
    e = sc.Expect(sc.line(qual=b"*") + sc.line(qual=b"") + sc.line(qual=b"III") + sc.line(qual=b"IIIII") + sc.line(qual=b"!#%'"))
    assert [r["quals"] for r in e.recs] == [b"!!!!", b"!!!!", b"!!!!", b"!!!!", b"!#%'"]
    assert [r["parsed"][5] for r in e.recs] == [8, 8, 16, 16, 0]
    text = sc.line(flag=b"16", qual=b"!#%'") + sc.line(flag=b"0", qual=b"!#%'") + sc.line(flag=b"16", qual=b"*")
    assert [r["quals"] for r in sc.Expect(text, sc.FINAL | sc.QUAL_FORWARD).recs] == [b"'%#!", b"!#%'", b"!!!!"]
    assert [r["quals"] for r in sc.Expect(text, sc.FINAL).recs] == [b"!#%'", b"!#%'", b"!!!!"]
    assert [r["strand"] for r in sc.Expect(text).recs] == [1, 0, 1]
    e = sc.Expect(sc.line(seq=b"*", qual=b"IIII") + sc.line(seq=b"*", qual=b"*"))
    assert [(r["bases"], r["quals"], r["parsed"][4], r["parsed"][5]) for r in e.recs] == [(b"", b"", 1, 4 | 16), (b"", b"", 1, 4 | 8)]


def test_the_expectation_of_a_small_file_by_hand():
    text = (b"@HD\tVN:1.6\n" + sc.line(b"a", b"0", b"chr", b"3", b"60", b"2S3M1I2M", b"ACGTACGT", b"IIIIIIII", (b"AS:i:11",))
            + sc.line(b"b", b"16", b"other", b"9", b"0", b"4M", b"ACGT", b"!#%'", (b"AS:i:8",)) + sc.line(b"c", b"4", b"*", b"0", b"0", b"*", b"AC", b"*", ()))
    e = sc.Expect(text, sc.FINAL | sc.QUAL_FORWARD, b"chr", 50)
    assert e.info == [3, 1, 14, 3, 4, len(text), 0, 0, 0, 1, 0, 2, 8]
    assert [r["status"] for r in e.recs] == [0, 2, 2]
    assert e.recs[0]["aln"] == (11, 2, 7, 2, 8, 50, 8, 4, 0) and e.recs[0]["ciglets"] == [(2, S), (3, M), (1, I), (2, M)]
    assert e.recs[1]["aln"] == (0,) * 9 and e.recs[1]["parsed"] == (9, 2, 16, 0, 0, sc.BIT_OTHER_RNAME) and e.recs[1]["quals"] == b"'%#!"
    assert e.recs[2]["parsed"] == (0, 3, 4, 0, 0, sc.BIT_NO_SCORE | sc.BIT_QUAL_MISSING)
    a = e.arrays()
    assert a["bases"] == b"ACGTACGTACGTAC" and list(a["offsets"]) == [0, 8, 12, 14] and a["qnames"] == b"abc" and list(a["inc"]) == [2, 3, 1, 2]
    # without rname record b is converted too (one more ciglet); without FINAL an unterminated last line is not parsed
    assert sc.Expect(text, 0).info[:6] == [3, 1, 14, 3, 5, len(text)] and sc.Expect(text[:-1], 0).info[:6] == [2, 1, 12, 2, 5, text[:-1].rfind(b"\n") + 1]


def revcomp(b: bytes) -> bytes:
    return b.translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


def test_round_trip_of_oracle_alignments_through_sam_lines(oracle):
    """sam_ref.sam_line over oracle alignments, both strands, with names and qualities, through the mirror: every record, ciglet,
    base, quality (with QUAL_FORWARD), name and strand byte is what went in, and score equals AS; no record is left out"""
    from zoe_amd.alignment import ALN_DTYPE

    rng = np.random.default_rng(11)
    ref = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=400).tobytes()
    scoring = oracle.dna_scoring(2, -5, b"N", -10, -1)
    reads, strands, alns = [], [], []
    for i in range(60):
        L = int(rng.integers(20, 90))
        p = int(rng.integers(0, len(ref) - L))
        r = bytearray(ref[p:p + L])
        for _ in range(int(rng.integers(0, 4))):
            k = int(rng.integers(0, len(r)))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                r[k] = b"ACGT"[(b"ACGT".index(r[k]) + 1) % 4]
            elif kind == 1:
                del r[k:k + 2]
            else:
                r[k:k] = b"GT"
        if i % 7 == 0:
            r = bytearray(b"N" * L)  # no alignment: an unmapped line
        if i % 5 == 0:
            r = bytearray(b"TTTTT") + r + bytearray(b"AAAA")  # soft clips on both ends
        read = bytes(r)
        strand = i & 1
        oriented = read  # the bases as aligned; a read of the reverse strand was given as its reverse complement
        reads.append(oriented)
        strands.append(strand)
        alns.append(oracle.align("i16", 16, scoring, oriented, ref))
    strands = [s if a.status == 0 else 0 for s, a in zip(strands, alns)]  # a read without an alignment has no strand
    recs = np.zeros(len(reads), dtype=ALN_DTYPE)
    inc, op, status = [], [], []
    for k, a in enumerate(alns):
        status.append(a.status)
        if a.status != 0:
            continue
        cig = [(int(n), ord(o)) for n, o in re.findall(r"(\d+)(\D)", a.cigar)]
        recs[k] = (a.score, a.ref_range[0], a.ref_range[1], a.query_range[0], a.query_range[1], a.ref_len, a.query_len, len(cig), len(inc))
        inc += [n for n, _ in cig]
        op += [o for _, o in cig]
    assert 0 in status and any(s != 0 for s in status) and any(o == S for o in op)
    inc, op = np.array(inc, dtype=np.uint32), np.array(op, dtype=np.uint8)
    names = [b"read:%d/x" % i for i in range(len(reads))]
    quals = [sc.qual_of(len(r), i) for i, r in enumerate(reads)]
    text = b"".join(sam_ref.sam_line(names[k], reads[k], quals[k], status[k], recs[k], inc, op, b"ref", 255, strands[k])[0] for k in range(len(reads)))
    e = sc.Expect(text, sc.FINAL | sc.QUAL_FORWARD, b"ref", len(ref))
    assert e.info[0] == len(reads) and e.info[6] == 0 and e.info[10] == 0
    a = e.arrays()
    assert a["bases"] == b"".join(reads) and a["quals"] == b"".join(quals) and a["qnames"] == b"".join(names)
    mapped = np.array(status) == 0
    assert np.array_equal(a["status"] == 0, mapped) and np.array_equal(a["status"][~mapped], np.full((~mapped).sum(), 2))
    assert np.array_equal(a["aln"][mapped], recs[mapped]) and np.array_equal(a["inc"], inc) and np.array_equal(a["op"], op)
    assert np.array_equal(a["strand"][mapped], np.array(strands, dtype=np.uint8)[mapped]) and not a["strand"][~mapped].any()  # an unmapped line has FLAG 4
    assert [int(r["parsed"][0]) for r in e.recs] == [int(recs[k]["ref_start"]) + 1 if mapped[k] else 0 for k in range(len(reads))]
