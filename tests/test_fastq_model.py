"""CPU checks of zsw_fastq_parse_batch (no GPU): the host model tests/models/fastq_parse.cpp — zoe_amd/csrc/zsw_fastq.hpp, the text
the kernels compile, behind a loop over the lanes, every array in a heap block of its exact size — against records.FastQReader on the
case list of tests/fastq_cases.py, under every flag set and at every misalignment of the text; once more through an
-fsanitize=address,undefined build of the model; the UTF-8 rule against bytes.decode on every short byte string; and the symbol in
every list."""
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import fastq_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_fastq.hpp")

_built = {}


def header_constant(name: str) -> int:
    return int(re.search(r"constexpr \w+ " + name + r" = (\d+);", open(HEADER).read()).group(1))


def model(sanitize: bool = False) -> str:
    if sanitize not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_fastq_"), "fastq_parse" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "models", "fastq_parse.cpp")], check=True)
        _built[sanitize] = exe
    return _built[sanitize]


def run(jobs, sanitize=False):
    """jobs: (flags, head, text) -> per job (info, bases, quals, names, offsets, name offsets)"""
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("".join(f"{flags} {head} {text.hex() or '-'}\n" for flags, head, text in jobs))
    try:
        out = subprocess.run([model(sanitize), f.name], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
    got = []
    for line in out.stdout.splitlines():
        w = line.split(" ")
        unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)
        got.append(([int(x) for x in w[:9]], unhex(w[9]), unhex(w[10]), unhex(w[11]), [int(x) for x in w[12].split(",")], [int(x) for x in w[13].split(",")]))
    assert len(got) == len(jobs)
    return got


def check(jobs, names, sanitize=False):
    for (flags, head, text), name, (info, bases, quals, qnames, off, noff) in zip(jobs, names, run(jobs, sanitize)):
        recs, want_info, _ = fc.expect(text, flags)
        w_bases, w_quals, w_off, w_names, w_noff = fc.arrays(recs)
        assert info == want_info, (name, flags, head, dict(zip(fc.INFO, info)), dict(zip(fc.INFO, want_info)))
        assert (bases, quals, qnames) == (w_bases, w_quals, w_names), (name, flags, head)
        assert off == list(w_off) and noff == list(w_noff), (name, flags, head)


def test_header_constants():
    assert header_constant("FQ_G") == 64 and header_constant("FQ_BLOCK_RECORDS") >= 1
    assert header_constant("FQ_TILE") == 16 * 64 * header_constant("FQ_TILE_SWEEPS")


def test_the_case_list_holds_what_it_claims():
    by_name = dict(fc.CASES)
    assert len(by_name) == len(fc.CASES)
    errors = {}
    for name, text in fc.CASES:
        recs, info, message = fc.expect(text)
        errors.setdefault(info[4], []).append((name, info[5]))
        assert (message is None) == (info[4] == 0)
    for code in range(1, 9):  # every code at record 0, in the middle and at the last record
        assert {at for _, at in errors[code]} >= {0, 2, 4}, code
    assert fc.expect(by_name["two_faults_in_one_record"])[1][4:6] == [fc.INVALID_UTF8, 2]
    assert fc.expect(by_name["two_bad_records"])[1][4:6] == [fc.MISSING_PLUS, 1]
    # a bare '\r' at the end of the file stays: `II\r` is three quality bytes, the last of them not a quality
    assert fc.expect(by_name["last_line_bare_cr"])[1][4:6] == [fc.INVALID_QUALITY, 1]
    assert fc.expect(by_name["last_line_bare_cr_mismatch"])[1][4:6] == [fc.LENGTH_MISMATCH, 1]
    assert fc.expect(by_name["valid_crlf_no_final_newline"])[0][-1] == (b"b", b"ACG", b"III")
    assert fc.expect(by_name["blank_line_after_last_record"])[1][3:6] == [len(by_name["blank_line_after_last_record"]) - 1, fc.MISSING_AT, 5]
    assert fc.expect(by_name["name_blanks"], fc.FINAL | fc.NAME_TO_BLANK)[0][2][0] == b"" and fc.expect(by_name["name_blanks"])[0][2][0] == b" lead"
    assert [len(s) for _, s, _ in fc.expect(by_name["seq_lengths"])[0]] == [1, 63, 64, 65, 127, 128, 129, 1000]
    assert [len(n) for n, _, _ in fc.expect(by_name["name_lengths"])[0]] == [1, 64, 255, 300]
    for k in (1, 2, 3):  # a file that stops inside its last record: an error with FINAL, a tail without
        text = by_name[f"stops_after_line{k}_unterminated"]
        assert fc.expect(text)[1][4] != 0 and fc.expect(text, 0)[1][:1] + fc.expect(text, 0)[1][4:5] == [5, 0]
    assert fc.expect(b"@x\nA\n+\nA")[1][0] == 1 and fc.expect(b"@x\nA\n+\nA", 0)[1][0] == 0


@pytest.mark.parametrize("flags", fc.FLAG_SETS)
def test_model_equals_reader_on_the_case_list(flags):
    jobs = [(flags, 0, text) for _, text in fc.CASES]
    check(jobs, [n for n, _ in fc.CASES])


def test_model_at_every_misalignment_and_the_tile_edges():
    tile = header_constant("FQ_TILE")
    jobs, names = [], []
    for name, text in fc.CASES[:12]:
        for head in range(1, 16):
            jobs.append((fc.FINAL, head, text))
            names.append(name)
    big = fc.mixed_file(60, 1, 400, seed=3)
    assert len(big) > 2 * tile + 17
    ends = [i for i, c in enumerate(big) if c == 10]
    for n in [0, 1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile]:
        for head in (0, 1, 15):
            for flags in (fc.FINAL, 0):
                jobs.append((flags, head, big[:n]))
                names.append(f"cut{n}")
    # a newline as the last byte of a tile, and as the first byte of the next one
    e = next(i for i in ends if i >= tile)
    for shift in (e - (tile - 1), e - tile):
        jobs.append((fc.FINAL, 0, big[shift:]))
        names.append(f"shift{shift}")
        assert big[shift:][tile - 1 if shift == e - (tile - 1) else tile] == 10
    check(jobs, names)


def test_model_without_final_cut_at_every_byte_of_the_last_two_records():
    text = fc.mixed_file(5, 3, 40, seed=5) + fc.rec(b"crlf one", b"ACGTAC", eol=b"\r\n") + fc.rec(b"last", b"ACG")
    ends = [i for i, c in enumerate(text) if c == 10]
    start = ends[-9] + 1
    jobs = [(0, 0, text[:n]) for n in range(start, len(text) + 1)]
    check(jobs, [f"cut{n}" for n in range(start, len(text) + 1)])
    for (flags, head, t), (info, *_rest) in zip(jobs, run(jobs)):
        full = sum(1 for i in ends if i < len(t)) // 4
        assert info[0] == full and info[3] == (ends[4 * full - 1] + 1 if full else 0)


def test_utf8_rule_equals_decode_on_every_short_string():
    """every string of up to three bytes from a set that holds every class of byte, and the four-byte forms: the header's rule
    against bytes.decode"""
    alphabet = [0x41, 0x7f, 0x80, 0x8f, 0x90, 0x9f, 0xa0, 0xbf, 0xc0, 0xc1, 0xc2, 0xdf, 0xe0, 0xe1, 0xec, 0xed, 0xee, 0xef, 0xf0, 0xf1, 0xf3, 0xf4, 0xf5, 0xff]
    strings = [bytes(t) for k in (1, 2, 3) for t in itertools.product(alphabet, repeat=k)]
    strings += [bytes((a, b, 0x80, c)) for a in (0xf0, 0xf1, 0xf4, 0xf5) for b in (0x80, 0x8f, 0x90, 0xbf, 0x41) for c in (0x80, 0xbf, 0x41, 0xc2)]
    jobs = [(fc.FINAL, 0, b"@" + s + b"\nA\n+\nI\n") for s in strings]
    got = run(jobs)
    for s, (info, *_rest) in zip(strings, got):
        try:
            s.decode("utf-8")
            want = 0
        except UnicodeDecodeError:
            want = fc.INVALID_UTF8
        assert info[4] == want, (s.hex(), info)


def test_model_under_the_host_sanitizers():
    jobs = [(flags, head, text) for _, text in fc.CASES for flags, head in ((fc.FINAL, 0), (0, 5), (fc.FINAL | fc.NAME_TO_BLANK, 15))]
    check(jobs, [n for n, _ in fc.CASES for _ in range(3)], sanitize=True)


def test_the_symbol_is_in_every_list():
    from zoe_amd import _lib

    assert "zsw_fastq_parse_batch" in _lib.SYMBOLS
    for rel in (("include", "zoe_sw.h"), ("include", "zoe_sw.hpp"), ("bindings", "rust", "zoe_sw_gpu.rs"), ("examples", "zsw_c_abi.c"), ("examples", "zsw_driver.cpp"),
                ("zoe_amd", "records.py"), ("INTEGRATION.md",), ("DESIGN.md",), ("README.md",)):
        assert "zsw_fastq_parse_batch" in open(os.path.join(ROOT, *rel)).read(), rel
    h = open(os.path.join(ROOT, "include", "zoe_sw.h")).read()
    for k, name in enumerate(fc.INFO):
        assert re.search(r"ZSW_FASTQ_INFO_" + name.upper() + r" = " + str(k) + r"\b", h), name
        assert getattr(_lib, "FASTQ_INFO_" + name.upper()) == k
    assert (fc.FINAL, fc.NAME_TO_BLANK) == (_lib.FASTQ_FINAL, _lib.FASTQ_NAME_TO_BLANK)
    assert np.array_equal([_lib.FASTQ_MISSING_AT, _lib.FASTQ_INVALID_QUALITY], [1, 8])
