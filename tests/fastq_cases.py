"""The case list of zsw_fastq_parse_batch's tests, as byte strings, and what the call must give for each: the records
`records.FastQReader` yields over the same bytes in front of its first FastQError, and which check raised. Nothing here knows the
device's rules; the expectation is the reader's own."""
import io

import numpy as np

from zoe_amd import records

FINAL, NAME_TO_BLANK = 1, 2
(MISSING_AT, MISSING_HEADER, INVALID_UTF8, MISSING_SEQUENCE, MISSING_PLUS, MISSING_QUALITY, LENGTH_MISMATCH, INVALID_QUALITY) = range(1, 9)
INFO = ("records", "bases", "name_bytes", "consumed", "error", "error_record", "error_offset", "min_len", "max_len")

# the reader's message for every check (zoe_amd/records.py), by how it begins
MESSAGES = (
    ("Missing '@' symbol", MISSING_AT), ("Missing FASTQ header", MISSING_HEADER), ("'utf-8' codec", INVALID_UTF8), ("Missing FASTQ sequence", MISSING_SEQUENCE),
    ("Missing '+' line", MISSING_PLUS), ("Missing FASTQ quality", MISSING_QUALITY), ("Sequence and quality score length mismatch", LENGTH_MISMATCH),
    ("Invalid quality score byte", INVALID_QUALITY),
)


def code_of(message: str) -> int:
    for prefix, code in MESSAGES:
        if message.startswith(prefix):
            return code
    raise AssertionError("unknown FastQError: " + message)


def parsed_part(text: bytes, final: bool) -> bytes:
    """the bytes a call looks at: all of them with FINAL, else the records whose four lines are all terminated"""
    if final:
        return text
    ends = [i for i, c in enumerate(text) if c == 10]
    n = len(ends) // 4
    return text[:ends[4 * n - 1] + 1] if n else b""


def expect(text: bytes, flags: int = FINAL):
    """-> (records as (name, bases, qualities) byte strings, the nine report words, the reader's message or None)"""
    f = io.BytesIO(parsed_part(text, bool(flags & FINAL)))
    reader = records.FastQReader(f)
    out, error, message = [], 0, None
    start = 0
    while True:
        start = f.tell()
        try:
            r = next(reader)
        except StopIteration:
            break
        except records.FastQError as e:
            message = str(e)
            error = code_of(message)
            break
        name = r.header.encode("utf-8")
        if flags & NAME_TO_BLANK:
            cut = [k for k, c in enumerate(name) if c in b" \t"]
            name = name[:cut[0]] if cut else name
        out.append((name, r.sequence, r.quality))
    lens = [len(s) for _, s, _ in out]
    info = [len(out), sum(lens), sum(len(n) for n, _, _ in out), start, error, len(out) if error else 0, start if error else 0, min(lens, default=0),
            max(lens, default=0)]
    return out, info, message


def arrays(recs):
    """the five output arrays of a call that delivers `recs`"""
    off = np.cumsum([0] + [len(s) for _, s, _ in recs]).astype(np.uint64)
    noff = np.cumsum([0] + [len(n) for n, _, _ in recs]).astype(np.uint64)
    return (b"".join(s for _, s, _ in recs), b"".join(q for _, _, q in recs), off, b"".join(n for n, _, _ in recs), noff)


def rec(name=b"r", seq=b"ACGT", qual=None, eol=b"\n", plus=b"+", last_eol=None):
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + plus + eol + qual + (eol if last_eol is None else last_eol)


def seq_of(n, k=0):
    return bytes(b"ACGTN"[(i * 7 + k) % 5] for i in range(n))


def qual_of(n, k=0):
    return bytes(33 + (i * 11 + k) % 94 for i in range(n))


FAULTS = {
    MISSING_AT: b"r\nACGT\n+\nIIII\n",
    MISSING_HEADER: b"@\nACGT\n+\nIIII\n",
    INVALID_UTF8: b"@r\x80\nACGT\n+\nIIII\n",
    MISSING_SEQUENCE: b"@r\n\n+\nIIII\n",
    MISSING_PLUS: b"@r\nACGT\n-\nIIII\n",
    MISSING_QUALITY: b"@r\nACGT\n+\n\n",
    LENGTH_MISMATCH: b"@r\nACGT\n+\nIII\n",
    INVALID_QUALITY: b"@r\nACGT\n+\nII I\n",
}


def five(bad: dict) -> bytes:
    """five records, those of `bad` (index -> bytes) in place of the good ones"""
    return b"".join(bad.get(i, rec(b"read%d extra" % i, seq_of(10 + i, i), qual_of(10 + i, i))) for i in range(5))


def cases():
    c = []
    good3 = [(b"a", b"ACGT"), (b"bb", b"ACGTACGTA"), (b"ccc", b"G")]
    c.append(("empty", b""))
    c.append(("valid_lf", b"".join(rec(n, s) for n, s in good3)))
    c.append(("valid_crlf", b"".join(rec(n, s, eol=b"\r\n") for n, s in good3)))
    c.append(("valid_no_final_newline", rec(b"a", b"ACGT") + rec(b"b", b"ACG", last_eol=b"")))
    c.append(("valid_crlf_no_final_newline", rec(b"a", b"ACGT", eol=b"\r\n") + rec(b"b", b"ACG", eol=b"\r\n", last_eol=b"")))
    c.append(("last_line_bare_cr", rec(b"a", b"ACGT") + rec(b"b", b"ACG", b"II\r", last_eol=b"")))
    c.append(("last_line_bare_cr_mismatch", rec(b"a", b"ACGT") + rec(b"b", b"AC", b"II\r", last_eol=b"")))
    c.append(("bare_cr_inside_a_line", rec(b"a\rb", b"AC\rT", b"II\rI")))
    c.append(("cr_cr_lf", b"@a\r\r\nAC\r\r\n+\r\r\nII\r\r\n"))
    c.append(("plus_name", rec(b"a", b"ACGT", plus=b"+a some more") + rec(b"b", b"AC", plus=b"+\t")))
    c.append(("name_blanks", rec(b"r1 first second", b"AC") + rec(b"r2\tx y", b"ACG") + rec(b" lead", b"A") + rec(b"\tlead", b"AT") + rec(b"tail ", b"ACGT") + rec(b" ", b"C")))
    c.append(("name_utf8", rec("ré".encode(), b"AC") + rec("€ uro".encode(), b"ACG") + rec("\U0001f9ec".encode(), b"A") + rec("x퟿\U0010ffff".encode("utf-8", "surrogatepass"), b"A")))
    for code, bad in FAULTS.items():
        for at in (0, 2, 4):
            c.append((f"code{code}_at{at}", five({at: bad})))
    c.append(("blank_line_as_header", five({1: b"\nACGT\n+\nIIII\n"})))
    c.append(("two_faults_in_one_record", five({2: b"@r\x80\n\n-\nII I\n"})))      # UTF-8 before sequence, plus, quality
    c.append(("two_faults_plus_and_quality", five({2: b"@r\nACGT\n-\nII\n"})))
    c.append(("two_faults_mismatch_and_quality", five({2: b"@r\nACGT\n+\nI I\n"})))
    c.append(("two_bad_records", five({3: FAULTS[INVALID_QUALITY], 1: FAULTS[MISSING_PLUS]})))
    c.append(("two_bad_records_late_first", five({4: FAULTS[MISSING_AT], 2: FAULTS[LENGTH_MISMATCH]})))
    for tag, bad in (("80", b"\x80"), ("c080", b"\xc0\x80"), ("eda080", b"\xed\xa0\x80"), ("f4908080", b"\xf4\x90\x80\x80"), ("truncated2", b"ab\xc3"), ("truncated3", b"ab\xe2\x82"),
                     ("truncated4", b"\xf0\x9f\xa7"), ("e08080", b"\xe0\x80\x80"), ("f0808080", b"\xf0\x80\x80\x80"), ("f5", b"\xf5\x80\x80\x80"), ("ff", b"a\xffb"),
                     ("lead_then_ascii", b"\xe2A\x82"), ("extra_continuation", b"\xc3\xa9\xa9"), ("at_byte_70", b"x" * 70 + b"\xc3"), ("across_sweep", b"x" * 62 + b"\xe2\x82")):
        c.append(("utf8_" + tag, five({1: rec(b"n" + bad, b"ACGT")})))
    c.append(("utf8_good_across_sweep", rec(b"x" * 62 + "€".encode() + b"y" * 70, b"ACGT") + rec(b"x" * 63 + "\U0001f9ec".encode(), b"AC")))
    c.append(("utf8_bad_behind_the_blank", five({1: rec(b"n x\x80", b"ACGT")})))
    for q in (0x20, 0x7f, 0x80):
        for where in ("first", "last"):
            qual = bytearray(qual_of(70))
            qual[0 if where == "first" else -1] = q
            c.append((f"quality_{q:02x}_{where}", five({3: rec(b"q", seq_of(70), bytes(qual))})))
    c.append(("quality_edges_good", rec(b"q", b"AC", b"!~")))
    c.append(("blank_line_after_last_record", five({}) + b"\n"))
    c.append(("two_blank_lines_after_last_record", five({}) + b"\n\n"))
    full = rec(b"last", b"ACGTA", b"IIIII")
    lines = full.split(b"\n")[:4]
    for k in (1, 2, 3):
        stop = b"\n".join(lines[:k])
        c.append((f"stops_after_line{k}", five({}) + stop + b"\n"))
        c.append((f"stops_after_line{k}_unterminated", five({}) + stop))
    c.append(("stops_inside_line4", five({}) + b"\n".join(lines[:3]) + b"\nII"))
    c.append(("only_a_header", b"@x"))
    c.append(("only_an_at", b"@"))
    c.append(("only_a_newline", b"\n"))
    c.append(("one_byte", b"A"))
    c.append(("shortest_record", b"@x\nA\n+\nA"))
    c.append(("shortest_records", b"@x\nA\n+\nA\n" * 7 + b"@x\nA\n+\nA"))
    c.append(("seq_lengths", b"".join(rec(b"s%d" % n, seq_of(n, n), qual_of(n, n)) for n in (1, 63, 64, 65, 127, 128, 129, 1000))))
    c.append(("name_lengths", b"".join(rec((b"n%d " % n + b"x" * n)[:n], b"ACGT") for n in (1, 64, 255, 300))))
    c.append(("crlf_long", b"".join(rec(b"s%d" % n, seq_of(n, n), qual_of(n, n), eol=b"\r\n") for n in (63, 64, 65, 300))))
    return c


CASES = cases()
FLAG_SETS = (FINAL, 0, FINAL | NAME_TO_BLANK, NAME_TO_BLANK)


def mixed_file(n, lo=1, hi=400, seed=1, name_width=None):
    """n good records of mixed lengths lo..hi"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    lens[:2] = (lo, hi)[:n]
    out = []
    for i, L in enumerate(lens):
        name = b"read_%d len=%d" % (i, L) if name_width is None else (b"r%0*d" % (name_width - 1, i))
        out.append(rec(name, seq_of(int(L), i), qual_of(int(L), i)))
    return b"".join(out)
