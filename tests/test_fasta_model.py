"""CPU checks of zsw_fasta_parse_batch (no GPU): the host model tests/models/fasta_parse.cpp — zoe_amd/csrc/zsw_fasta.hpp, the text
the kernels compile, behind a loop over the lanes, every array in a heap block of its exact size — against records.FastaReader on the
case list of tests/fasta_cases.py, under every flag set and at every misalignment of the text; once more through an
-fsanitize=address,undefined build of the model; records.FastaReader against the known answers of the reference's own tests
(tests/golden/fasta_known_answers.json); and the symbol and its constants in every list."""
import io
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import fasta_cases as fc
from zoe_amd import records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_text.hpp")

_built = {}


def header_constant(name: str) -> int:
    return int(re.search(r"constexpr \w+ " + name + r" = (\d+);", open(HEADER).read()).group(1))


def model(sanitize: bool = False) -> str:
    if sanitize not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_fasta_"), "fasta_parse" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "models", "fasta_parse.cpp")], check=True)
        _built[sanitize] = exe
    return _built[sanitize]


def run(jobs, sanitize=False):
    """jobs: (flags, head, text) -> per job (info, bases, names, offsets, name offsets), or None for "invalid\""""
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("".join(f"{flags} {head} {text.hex() or '-'}\n" for flags, head, text in jobs))
    try:
        out = subprocess.run([model(sanitize), f.name], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
    got = []
    for line in out.stdout.splitlines():
        if line == "invalid":
            got.append(None)
            continue
        w = line.split(" ")
        unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)
        got.append(([int(x) for x in w[:9]], unhex(w[9]), unhex(w[10]), [int(x) for x in w[11].split(",")], [int(x) for x in w[12].split(",")]))
    assert len(got) == len(jobs)
    return got


def check(jobs, names, sanitize=False):
    for (flags, head, text), name, (info, bases, qnames, off, noff) in zip(jobs, names, run(jobs, sanitize)):
        recs, want_info, _ = fc.expect(text, flags)
        w_bases, w_off, w_names, w_noff = fc.arrays(recs)
        assert info == want_info, (name, flags, head, dict(zip(fc.INFO, info)), dict(zip(fc.INFO, want_info)))
        assert (bases, qnames) == (w_bases, w_names), (name, flags, head)
        assert off == list(w_off) and noff == list(w_noff), (name, flags, head)


def test_reader_reproduces_the_known_answers():
    cases = fc.golden()
    assert len(cases) == 14  # thirteen tests, one of them with two inputs
    for c in cases:
        got, message = [], None
        try:
            for r in records.FastaReader(io.BytesIO(c["text"].encode())):
                got.append([r.name.decode(), r.sequence.decode()])
        except records.FastaError as e:
            message = str(e)
        assert got == c["records"] and message == c["error"], (c["name"], got, message)
    with pytest.raises(records.FastaError, match="No FASTA data was found!"):
        records.FastaReader.from_readable(io.BytesIO(b""))


def test_the_case_list_holds_what_it_claims():
    by_name = dict(fc.CASES)
    assert len(by_name) == len(fc.CASES)
    errors = {}
    for name, text in fc.CASES:
        recs, info, message = fc.expect(text)
        errors.setdefault(info[4], []).append((name, info[5]))
        assert (message is None) == (info[4] == 0)
    for code in (fc.MISSING_HEADER, fc.GT_IN_HEADER, fc.MISSING_SEQUENCE, fc.GT_IN_SEQUENCE):  # as record 0, in the middle and as the last record
        assert {at for _, at in errors[code]} >= {0, 2, 4}, code
    assert errors[fc.NO_DATA] and errors[fc.MISSING_GT]
    e = lambda name, flags=fc.FINAL: fc.expect(by_name[name], flags)
    # the quirk: a later record without a '\n' and without a sequence byte that ends at '>' is GT_IN_HEADER, with a '\n' MISSING_SEQUENCE
    assert e("cr_gt_quirk")[1][4:7] == [fc.GT_IN_HEADER, 1, 5] and e("cr_run_then_gt")[1][4] == fc.GT_IN_HEADER
    assert e("cr_gt_quirk_with_newline")[1][4] == fc.MISSING_SEQUENCE and e("cr_then_newline_then_gt")[1][4] == fc.MISSING_SEQUENCE
    assert e("cr_gt_first_record")[1][4] == fc.GT_IN_HEADER and e("cr_gt_in_sequence")[1][4:6] == [fc.GT_IN_SEQUENCE, 0]
    assert e("gt_gt_first")[1][4] == fc.GT_IN_HEADER and e("gt_gt_later")[1][4:6] == [fc.GT_IN_HEADER, 1]
    assert e("gt_newline_gt")[1][4:6] == [fc.MISSING_HEADER, 1] and e("gt_last_byte")[1][4:6] == [fc.MISSING_HEADER, 1]
    # line breaks: the first header runs to its '\n', a later one ends at a lone '\r'
    assert e("lone_cr_in_first_header")[0][0] == (b"a\rb", b"ACGT") and e("lone_cr_ends_a_later_header")[0][1] == (b"b", b"GGTT")
    assert e("cr_cr_lf_first_header")[0][0][0] == b"a\r" and e("cr_cr_lf_later_header")[0][1] == (b"b", b"AC")
    assert e("first_header_only_cr")[0] == [(b"\r", b"ACGT")] and e("first_header_crlf_empty")[1][4] == fc.MISSING_HEADER
    assert e("blank_lines_in_bodies")[0] == [(b"a", b"ACGT"), (b"b", b"A")]
    assert e("sequence_bytes")[0][0][1] == b"ac gt\tNn*-\x00\x80\xff\x0b"
    # the start of the file: '\x0b' is no whitespace, a '>' behind a blank or a '\r' does not start its line
    for name, at in (("space_before_gt", 1), ("tab_before_gt", 2), ("cr_before_gt", 1), ("vt_line_first", 0), ("vt_before_gt", 1), ("text_first", 2), ("text_after_blanks_no_gt", 5)):
        assert e(name)[1][3:7] == [0, fc.MISSING_GT, 0, at] and e(name, 0)[1][3:7] == [0, fc.MISSING_GT, 0, at], name
    assert e("blank_lines_first")[1][:2] == [1, 4] and e("only_whitespace_unterminated")[1][4] == fc.NO_DATA
    assert e("only_whitespace_unterminated", 0)[1] == [0, 0, 0, 5, 0, 0, 0, 0, 0] and e("empty", 0)[1][3:5] == [0, 0]
    # names
    assert [n for n, _ in e("name_blanks", fc.FINAL | fc.NAME_TO_BLANK)[0]] == [b"r1", b"r2", b"", b"", b"tail", b"", b""]
    assert e("name_high_bytes")[0][1][0] == b"\x80\xff bad utf8"
    # without FINAL the record at the last '>' waits for the next buffer, whatever it looks like
    assert e("gt_last_byte", 0)[1] == [1, 4, 1, 8, 0, 0, 0, 4, 4] and e("shortest_record", 0)[1][:5] == [0, 0, 0, 0, 0]
    assert e("gt_last_byte_after_base", 0)[1][4:6] == [fc.GT_IN_SEQUENCE, 0]
    assert [len(s) for _, s in e("wrapped")[0]] == [1, 59, 60, 61, 127, 128, 129, 1000]


@pytest.mark.parametrize("flags", fc.FLAG_SETS)
def test_model_equals_reader_on_the_case_list(flags):
    jobs = [(flags, 0, text) for _, text in fc.CASES]
    check(jobs, [n for n, _ in fc.CASES])


@pytest.mark.parametrize("flags", [f | fc.CONTINUED for f in fc.FLAG_SETS])
def test_model_equals_reader_on_continued_texts(flags):
    cont = fc.continued_cases()
    assert len(cont) > 100
    check([(flags, 0, text) for _, text in cont], [n for n, _ in cont])
    assert run([(flags, 0, b""), (flags, 3, b"a>b\nA\n"), (flags, 0, b"\n>b\nA\n")]) == [None, None, None]


def edge_texts(tile):
    """(what, text, head): each of these as the last byte of a tile and as the first byte of the next — a '>', the '\\n' of a
    "\\r\\n", the last byte of a header, the first kept byte of a body — in the first tile edge and, with a long single line, the third"""
    tail = b">hdr name\r\nACGT\r\nAC\r\n>z\r\nA\r\n"
    out = []
    for what, idx in (("gt", 0), ("header_end", 8), ("crlf", 10), ("first_base", 11)):
        assert {"gt": b">", "header_end": b"e", "crlf": b"\n", "first_base": b"A"}[what][0] == tail[idx]
        for edge in (tile, 3 * tile):
            for v in (edge - 1, edge):
                for head in (0, 5):
                    text = b">p\r\n" + fc.seq_of(v - head - 6 - idx) + b"\r\n" + tail
                    assert text[v - head] == tail[idx]
                    out.append((f"{what}_at{v}_head{head}", text, head))
    return out


def test_model_at_every_misalignment_and_the_tile_edges():
    tile = header_constant("FQ_TILE")
    jobs, names = [], []
    for name, text in fc.CASES:
        for head in range(1, 16):
            jobs.append((fc.FINAL, head, text))
            names.append(name)
    big = fc.mixed_file(40, 1, 700, seed=3)
    assert len(big) > 2 * tile + 17
    for n in [0, 1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile]:
        for head in (0, 1, 15):
            for flags in (fc.FINAL, 0):
                jobs.append((flags, head, big[:n]))
                names.append(f"cut{n}")
    for what, text, head in edge_texts(tile):
        for flags in (fc.FINAL, fc.FINAL | fc.CONTINUED, fc.NAME_TO_BLANK):
            jobs.append((flags, head, text))
            names.append(what)
    check(jobs, names)


def test_model_without_final_cut_at_every_byte_of_the_last_two_records():
    text = fc.mixed_file(5, 3, 90, seed=5, width=20) + fc.rec(b"crlf one", b"ACGTACGTAC", eol=b"\r\n", width=4) + fc.rec(b"last", b"ACG")
    gts = [i for i, c in enumerate(text) if c == 62]
    start = gts[-2]
    jobs = [(0, 0, text[:n]) for n in range(start, len(text) + 1)]
    check(jobs, [f"cut{n}" for n in range(start, len(text) + 1)])
    whole = fc.expect(text)[0]
    for (flags, head, t), (info, *_rest) in zip(jobs, run(jobs)):
        full = sum(1 for i in gts if i < len(t)) - 1
        assert info[0] == full and info[3] == gts[full] and info[4] == 0
        # the restart at CONSUMED, as a continued text: together the records of the whole file
        rest = fc.expect(text[info[3]:], fc.FINAL | fc.CONTINUED)
        assert fc.expect(t, 0)[0] + rest[0] == whole and rest[1][4] == 0


def test_model_equals_reader_on_random_texts():
    """short strings over the bytes the rules look at: every arrangement of '>', line breaks, blanks and bases the reader can meet"""
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b">>\n\n\r A\t\x0bC", dtype=np.uint8)
    texts = [bytes(rng.choice(alphabet, size=int(rng.integers(0, 24)))) for _ in range(4000)]
    for flags in (fc.FINAL, 0, fc.FINAL | fc.NAME_TO_BLANK):
        check([(flags, int(rng.integers(0, 16)), t) for t in texts], [t.hex() for t in texts])
    cont = [b">" + t for t in texts]
    for flags in (fc.FINAL | fc.CONTINUED, fc.CONTINUED):
        check([(flags, 0, t) for t in cont], [t.hex() for t in cont])


def test_model_under_the_host_sanitizers():
    jobs = [(flags, head, text) for _, text in fc.CASES for flags, head in ((fc.FINAL, 0), (0, 5), (fc.FINAL | fc.NAME_TO_BLANK, 15))]
    check(jobs, [n for n, _ in fc.CASES for _ in range(3)], sanitize=True)
    cont = fc.continued_cases()
    check([(fc.CONTINUED, 9, text) for _, text in cont], [n for n, _ in cont], sanitize=True)
    big = fc.mixed_file(40, 1, 700, seed=3)
    check([(fc.FINAL, 3, big), (0, 0, big[:5000])], ["big", "big_cut"], sanitize=True)


def test_the_symbol_and_its_constants_are_in_every_list():
    from zoe_amd import _lib

    assert "zsw_fasta_parse_batch" in _lib.SYMBOLS
    for rel in (("include", "zoe_sw.h"), ("include", "zoe_sw.hpp"), ("bindings", "rust", "zoe_sw_gpu.rs"), ("examples", "zsw_c_abi.c"), ("zoe_amd", "records.py"),
                ("INTEGRATION.md",), ("DESIGN.md",), ("README.md",)):
        assert "zsw_fasta_parse_batch" in open(os.path.join(ROOT, *rel)).read(), rel
    assert "FastaReader" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    h = open(os.path.join(ROOT, "include", "zoe_sw.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "zoe_sw_gpu.rs")).read()
    hpp = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_fasta.hpp")).read()
    for k, name in enumerate(fc.INFO):
        assert re.search(r"ZSW_FASTA_INFO_" + name.upper() + r" = " + str(k) + r"\b", h), name
        assert getattr(_lib, "FASTA_INFO_" + name.upper()) == k
    assert re.search(r"ZSW_FASTA_INFO_WORDS = 9\b", h) and re.search(r"ZSW_FASTA_INFO_WORDS: usize = 9;", rs) and _lib.FASTA_INFO_WORDS == 9
    for k, name in enumerate(("NO_DATA", "MISSING_GT", "MISSING_HEADER", "GT_IN_HEADER", "MISSING_SEQUENCE", "GT_IN_SEQUENCE"), start=1):
        assert re.search(r"ZSW_FASTA_" + name + r" = " + str(k) + r"\b", h), name
        assert re.search(r"ZSW_FASTA_" + name + r": u64 = " + str(k) + r";", rs), name
        assert re.search(r"\b" + name + r" = " + str(k) + r"\b", hpp), name
        assert getattr(_lib, "FASTA_" + name) == k == getattr(fc, name)
    for k, name in ((1, "FINAL"), (2, "NAME_TO_BLANK"), (4, "CONTINUED")):
        assert re.search(r"ZSW_FASTA_" + name + r" = " + str(k) + r"\b", h) and re.search(r"ZSW_FASTA_" + name + r": i32 = " + str(k) + r";", rs), name
        assert getattr(_lib, "FASTA_" + name) == k == getattr(fc, name)
