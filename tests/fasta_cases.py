"""The case list of zsw_fasta_parse_batch's tests, as byte strings, and what the call must give for each: the records
`records.FastaReader` yields over the same bytes in front of its first FastaError, and which check raised. Nothing here knows the
device's rules; the expectation is the reader's own."""
import io
import json
import os

import numpy as np

from zoe_amd import records

FINAL, NAME_TO_BLANK, CONTINUED = 1, 2, 4
(NO_DATA, MISSING_GT, MISSING_HEADER, GT_IN_HEADER, MISSING_SEQUENCE, GT_IN_SEQUENCE) = range(1, 7)
INFO = ("records", "bases", "name_bytes", "consumed", "error", "error_record", "error_offset", "min_len", "max_len")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fasta_known_answers.json")


def golden():
    return json.load(open(GOLDEN))["cases"]


def expect(text: bytes, flags: int = FINAL):
    """-> (records as (name, bases) byte strings, the nine report words, the reader's message or None). Without FINAL the record
    that starts at the last '>' is the reader's to read once the rest of the file is there: its outcome is dropped, and so is "no
    data"; with CONTINUED the reader starts as one that has just read the '>' in front of a later record."""
    gts = [i for i, c in enumerate(text) if c == 62]
    final = bool(flags & FINAL)
    budget = len(gts) if final else max(len(gts) - 1, 0)  # the records this call may parse
    reader = records.FastaReader(io.BytesIO(text), continued=bool(flags & CONTINUED))
    out, error, message, at = [], 0, None, 0
    consumed = len(text) if final else (gts[-1] if gts else text.rfind(b"\n") + 1)
    while True:
        try:
            r = next(reader)
        except StopIteration:
            break
        except records.FastaError as e:
            if e.code == MISSING_GT or (e.code == NO_DATA and final) or (e.code != NO_DATA and len(out) < budget):
                message, error, at = str(e), e.code, e.offset
                consumed = 0 if e.code in (NO_DATA, MISSING_GT) else e.offset
            break
        if len(out) == budget:
            break
        name = r.name
        if flags & NAME_TO_BLANK:
            cut = [k for k, c in enumerate(name) if c in b" \t"]
            name = name[:cut[0]] if cut else name
        out.append((name, r.sequence))
    lens = [len(s) for _, s in out]
    info = [len(out), sum(lens), sum(len(n) for n, _ in out), consumed, error, len(out) if error else 0, at if error else 0, min(lens, default=0), max(lens, default=0)]
    return out, info, message


def arrays(recs):
    """the four output arrays of a call that delivers `recs`"""
    off = np.cumsum([0] + [len(s) for _, s in recs]).astype(np.uint64)
    noff = np.cumsum([0] + [len(n) for n, _ in recs]).astype(np.uint64)
    return (b"".join(s for _, s in recs), off, b"".join(n for n, _ in recs), noff)


def seq_of(n, k=0):
    return bytes(b"ACGTN"[(i * 7 + k) % 5] for i in range(n))


def wrap(seq: bytes, width: int, eol: bytes = b"\n") -> bytes:
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def rec(name=b"r", seq=b"ACGT", eol=b"\n", width=None, last_eol=None):
    body = wrap(seq, width or max(len(seq), 1), eol)
    if last_eol is not None:
        body = body[:len(body) - len(eol)] + last_eol
    return b">" + name + eol + body


# one record that fails with each code where it stands as record 0 of the file / as a later record
FAULTS_FIRST = {
    MISSING_HEADER: b">\nACGT\n",
    GT_IN_HEADER: b">a>b\nACGT\n",
    MISSING_SEQUENCE: b">a\n\r\n\n",
    GT_IN_SEQUENCE: b">a\nAC>GT\n",
}
FAULTS_LATER = {
    MISSING_HEADER: b">\r\nACGT\n",
    GT_IN_HEADER: b">a>b\nACGT\n",
    MISSING_SEQUENCE: b">a\n\n",
    GT_IN_SEQUENCE: b">a\nACGT",  # the next '>' follows a base
}


def five(bad: dict, tail: bytes = b"") -> bytes:
    """five records, those of `bad` (index -> bytes) in place of the good ones"""
    return b"".join(bad.get(i, rec(b"read%d extra words" % i, seq_of(10 + 13 * i, i), width=7 + i)) for i in range(5)) + tail


def cases():
    c = [("golden_" + g["name"], g["text"].encode()) for g in golden()]
    good3 = [(b"a", b"ACGT"), (b"bb", b"ACGTACGTA"), (b"ccc", b"G")]
    c.append(("empty", b""))
    c.append(("valid_lf", b"".join(rec(n, s) for n, s in good3)))
    c.append(("valid_crlf", b"".join(rec(n, s, eol=b"\r\n", width=3) for n, s in good3)))
    c.append(("valid_no_final_newline", rec(b"a", b"ACGT") + rec(b"b", b"ACG", last_eol=b"")))
    c.append(("valid_crlf_no_final_newline", rec(b"a", b"ACGT", eol=b"\r\n") + rec(b"b", b"ACG", eol=b"\r\n", last_eol=b"")))
    c.append(("shortest_record", b">a\nA"))
    c.append(("shortest_records", b">a\nA\n" * 9 + b">a\nA"))
    c.append(("wrapped", b"".join(rec(b"s%d" % n, seq_of(n, n), width=60) for n in (1, 59, 60, 61, 127, 128, 129, 1000))))
    c.append(("wrapped_crlf", b"".join(rec(b"s%d" % n, seq_of(n, n), eol=b"\r\n", width=60) for n in (59, 60, 61, 300))))
    c.append(("single_lines", b"".join(rec(b"s%d" % n, seq_of(n, n)) for n in (1, 63, 64, 65, 127, 128, 129, 1000))))
    c.append(("name_lengths", b"".join(rec((b"n%d " % n + b"x" * n)[:n], b"ACGT") for n in (1, 64, 255, 300))))
    # line breaks of every kind
    c.append(("lone_cr_in_first_header", b">a\rb\nACGT\n>c\nAC\n"))                    # the first header runs to its '\n': the '\r' stays in the name
    c.append(("lone_cr_ends_a_later_header", b">a\nACGT\n>b\rGG\nTT\n"))               # a later header ends at the '\r': GG is sequence
    c.append(("lone_cr_in_bodies", b">a\nAC\rGT\r\r\nA\n>b\nA\rC\r"))
    c.append(("cr_cr_lf_first_header", b">a\r\r\nACGT\n"))                              # one '\r' is chopped, one stays
    c.append(("cr_cr_lf_later_header", b">a\nACGT\n>b\r\r\nAC\n"))
    c.append(("first_header_only_cr", b">\r\r\nACGT\n"))                                # the name is one '\r'
    c.append(("first_header_crlf_empty", b">\r\nACGT\n"))
    c.append(("blank_lines_in_bodies", b">a\n\n\nAC\n\n\r\nGT\n\n>b\r\n\r\n\r\nA\r\n\r\n"))
    c.append(("cr_gt_quirk", b">a\nA\n>b\r>c\nA\n"))                                    # GT_IN_HEADER although the '\r' ended the header
    c.append(("cr_gt_quirk_with_newline", b">a\nA\n>b\r\n>c\nA\n"))                     # MISSING_SEQUENCE
    c.append(("cr_then_newline_then_gt", b">a\nA\n>b\r\r\r\n>c\nA\n"))
    c.append(("cr_run_then_gt", b">a\nA\n>b\r\r\r>c\nA\n"))
    c.append(("cr_gt_in_sequence", b">a\nAC\r>b\nA\n"))                                 # "\r>" is no line start
    c.append(("cr_gt_first_record", b">a\r>c\nA\n"))
    c.append(("gt_gt_first", b">>a\nA\n"))
    c.append(("gt_gt_later", b">a\nA\n>>b\nA\n"))
    c.append(("gt_newline_gt", b">a\nA\n>\n>b\nA\n"))
    c.append(("gt_last_byte", b">a\nACGT\n>"))
    c.append(("gt_last_byte_after_base", b">a\nACGT>"))
    c.append(("only_a_gt", b">"))
    c.append(("only_gt_newline", b">\n"))
    c.append(("header_without_line_break_at_the_end", b">a\nACGT\n>bcd"))
    c.append(("first_header_without_line_break", b">abc"))
    c.append(("first_header_ends_with_cr", b">abc\r"))
    c.append(("later_header_ends_with_cr", b">a\nA\n>abc\r"))
    # the start of the file
    c.append(("blank_lines_first", b"\n\r\n \t\n\x0c\n>a\nACGT\n"))
    c.append(("space_before_gt", b" >a\nACGT\n"))
    c.append(("tab_before_gt", b"\n\t>a\nACGT\n"))
    c.append(("cr_before_gt", b"\r>a\nACGT\n"))
    c.append(("vt_line_first", b"\x0b\n>a\nACGT\n"))
    c.append(("vt_before_gt", b"\n\x0b>a\nACGT\n"))
    c.append(("text_first", b"\n\nACGT\n>a\nACGT\n"))
    c.append(("text_after_blanks_no_gt", b"  \n  x"))
    c.append(("only_whitespace_unterminated", b" \n\t\r\n  "))
    c.append(("only_newlines", b"\n\n\n"))
    c.append(("one_byte", b"A"))
    c.append(("one_newline", b"\n"))
    # names
    c.append(("name_blanks", rec(b"r1 first second", b"AC") + rec(b"r2\tx y", b"ACG") + rec(b" lead", b"A") + rec(b"\tlead", b"AT") + rec(b"tail ", b"ACGT") + rec(b" ", b"C")
              + rec(b"  \t ", b"GG")))
    c.append(("name_high_bytes", rec(b"r\xc3\xa9", b"AC") + rec(b"\x80\xff bad utf8", b"ACG") + rec(b"x\xed\xa0\x80", b"A")))
    c.append(("sequence_bytes", rec(b"s", b"ac gt\tNn*-\x00\x80\xff\x0b", width=5) + rec(b"t", b" ")))
    for code in (MISSING_HEADER, GT_IN_HEADER, MISSING_SEQUENCE, GT_IN_SEQUENCE):
        c.append((f"code{code}_at0", five({0: FAULTS_FIRST[code]})))
        for at in (2, 4):
            c.append((f"code{code}_at{at}", five({at: FAULTS_LATER[code]}, tail=b">z\nA\n" if code == GT_IN_SEQUENCE else b"")))
    c.append(("code5_at4_end_of_text", five({4: b">a"})))
    c.append(("code5_at4_only_breaks", five({4: b">a\r\n\r\n\n"})))
    c.append(("code3_at4_end_of_text", five({4: b">"})))
    c.append(("two_bad_records", five({3: FAULTS_LATER[MISSING_SEQUENCE], 1: FAULTS_LATER[MISSING_HEADER]})))
    c.append(("two_bad_records_late_first", five({4: FAULTS_LATER[GT_IN_HEADER], 2: FAULTS_LATER[MISSING_SEQUENCE]})))
    c.append(("bad_start_and_bad_record", b"x\n" + five({1: FAULTS_LATER[MISSING_HEADER]})))
    return c


CASES = cases()
FLAG_SETS = (FINAL, 0, FINAL | NAME_TO_BLANK, NAME_TO_BLANK)


def continued_cases():
    """(name, text) whose text starts at the '>' of a later record: every case's text from each of its '>' on"""
    out = []
    for name, text in CASES:
        for k, i in enumerate(j for j, ch in enumerate(text) if ch == 62):
            if i and k <= 3:
                out.append((f"{name}_from{i}", text[i:]))
    return out


def mixed_file(n, lo=1, hi=400, seed=1, width=60, eol=b"\n"):
    """n good records of mixed lengths lo..hi, wrapped at `width` columns"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    lens[:2] = (lo, hi)[:n]
    return b"".join(rec(b"read_%d len=%d" % (i, L), seq_of(int(L), i), eol=eol, width=width) for i, L in enumerate(lens))
