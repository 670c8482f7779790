"""CPU checks of zsw_sam_parse_batch (no GPU): the host model tests/models/samtext_parse.cpp — zoe_amd/csrc/zsw_samtext.hpp, the text
the kernels compile, behind a loop over the lanes, every array in a heap block of its exact size — against the mirror of the reference
in zoe_amd/records.py (SAMReader, SamData.is_unmapped / to_alignment / score) on the case list of tests/samtext_cases.py, under every
flag set, with and without rname, at every misalignment of the text and at the tile edges; without FINAL cut at every byte of the last
two lines; once more through an -fsanitize=address,undefined build of the model (a stand-alone program run as a subprocess); and
the symbol and the constants in every list."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import samtext_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_samtext.hpp")
FQ_HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_fastq.hpp")

_built = {}


def header_constant(name: str, path: str = HEADER) -> int:
    return int(re.search(r"constexpr \w+ " + name + r" = (\d+);", open(path).read()).group(1))


def model(sanitize: bool = False) -> str:
    if sanitize not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_samtext_"), "samtext_parse" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "models", "samtext_parse.cpp")], check=True)
        _built[sanitize] = exe
    return _built[sanitize]


def run(jobs, sanitize=False):
    """jobs: (flags, head, ref_len, rname or None, text) -> per job a dict of the report and the output arrays"""
    hx = lambda b: b.hex() if b else "-"
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("".join(f"{flags} {head} {ref_len} {hx(rname)} {hx(text)}\n" for flags, head, ref_len, rname, text in jobs))
    try:
        out = subprocess.run([model(sanitize), f.name], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
    got = []
    unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)
    tuples = lambda s: [] if s == "-" else [tuple(int(x) for x in t.split(":")) for t in s.split(",")]
    for row in out.stdout.splitlines():
        w = row.split(" ")
        got.append(dict(info=[int(x) for x in w[:13]], bases=unhex(w[13]), quals=unhex(w[14]), qnames=unhex(w[15]), offsets=[int(x) for x in w[16].split(",")],
                        qname_offsets=[int(x) for x in w[17].split(",")], recs=tuples(w[18]), ciglets=tuples(w[19]), strand=[t[0] for t in tuples(w[20])],
                        parsed=tuples(w[21])))
    assert len(got) == len(jobs)
    return got


def check(jobs, names, sanitize=False):
    for (flags, head, ref_len, rname, text), name, got in zip(jobs, names, run(jobs, sanitize)):
        want = sc.Expect(text, flags, rname, ref_len)
        what = (name, flags, head, rname)
        assert got["info"] == want.info, (what, dict(zip(sc.INFO, got["info"])), dict(zip(sc.INFO, want.info)))
        a = want.arrays()
        assert (got["bases"], got["quals"], got["qnames"]) == (a["bases"], a["quals"], a["qnames"]), what
        assert got["offsets"] == list(a["offsets"]) and got["qname_offsets"] == list(a["qname_offsets"]), what
        assert [r[0] for r in got["recs"]] == [r["status"] for r in want.recs], what
        assert [r[1:] for r in got["recs"]] == [r["aln"] for r in want.recs], (what, got["recs"], [r["aln"] for r in want.recs])
        assert got["ciglets"] == [c for r in want.recs for c in r["ciglets"]], what
        assert got["strand"] == [r["strand"] for r in want.recs], what
        assert got["parsed"] == [r["parsed"] for r in want.recs], (what, got["parsed"], [r["parsed"] for r in want.recs])


def test_header_constants():
    assert header_constant("SAM_FIELDS") == 11 and header_constant("SAM_BLOCK_LINES") >= 1
    assert header_constant("FQ_G", FQ_HEADER) == 64
    import ctypes

    from zoe_amd import _lib
    from zoe_amd.alignment import PARSED_DTYPE

    assert ctypes.sizeof(_lib.ZswSamParsed) == 24 == PARSED_DTYPE.itemsize and [f[0] for f in _lib.ZswSamParsed._fields_] == list(PARSED_DTYPE.names)
    assert ctypes.sizeof(_lib.ZswSamParseOut) == 15 * 8


def test_the_case_list_holds_what_it_claims():
    by_name = dict(sc.CASES)
    assert len(by_name) == len(sc.CASES)
    errors = {}
    for name, text in sc.CASES:
        e = sc.Expect(text)
        errors.setdefault(e.info[6], []).append(e.info[7])
    for code in range(1, 7):  # every reader code at the first line, in the middle and at the last line
        assert set(errors[code]) >= {0, 2, 4}, code
    codes = {r["parsed"][4] for _, text in sc.CASES for r in sc.Expect(text).recs}
    assert codes >= set(range(0, 11))
    bits = 0
    for _, text in sc.CASES:
        for r in sc.Expect(text, sc.FINAL, b"chr").recs:
            bits |= r["parsed"][5]
    assert bits == 31
    assert max(len(r["ciglets"]) for _, text in sc.CASES for r in sc.Expect(text).recs) >= 32
    assert [len(r["bases"]) for r in sc.Expect(by_name["seq_lengths"]).recs] == [1, 63, 64, 65, 1000]


@pytest.mark.parametrize("flags", sc.FLAG_SETS)
@pytest.mark.parametrize("rname", [None, b"chr"])
def test_model_equals_mirror_on_the_case_list(flags, rname):
    jobs = [(flags, 0, 77, rname, text) for _, text in sc.CASES]
    check(jobs, [n for n, _ in sc.CASES])


def test_model_at_every_misalignment_and_the_tile_edges():
    tile = header_constant("FQ_TILE", FQ_HEADER)
    jobs, names = [], []
    for name, text in sc.CASES[1:14]:
        for head in range(1, 16):
            jobs.append((sc.FINAL | sc.QUAL_FORWARD, head, 5, b"chr", text))
            names.append(name)
    big = sc.mixed_file(40, seed=3)
    assert len(big) > 2 * tile + 17
    for n in [0, 1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile]:
        for head in (0, 1, 15):
            for flags in (sc.FINAL, 0):
                jobs.append((flags, head, 0, None, big[:n]))
                names.append(f"cut{n}")
    # a tab, a newline and a CIGAR op as the last byte of a tile and as the first byte of the next one
    special = sc.line(qname=b"edge", cigar=b"3M2I" * 8, seq=sc.seq_of(40))
    g, base_len = sc.good(0), len(sc.line(qname=b""))
    for what, off in (("tab", special.index(b"\t")), ("newline", len(special) - 1), ("op", special.index(b"3M2I") + 1)):
        for at in (tile - 1, tile):
            k = (at - off - base_len - 1) // len(g)
            pad = at - off - base_len - k * len(g)
            text = sc.line(qname=b"p" * pad) + g * k + special + g * 2
            assert pad >= 1 and text[at] == special[off] and text[at - off:at - off + len(special)] == special
            jobs.append((sc.FINAL, 0, 9, None, text))
            names.append(f"{what}_at{at}")
    check(jobs, names)


def test_model_without_final_cut_at_every_byte_of_the_last_two_lines():
    text = sc.mixed_file(6, seed=5, max_read=40) + sc.good(2).replace(b"\n", b"\r\n") + sc.good(3)
    ends = [i for i, c in enumerate(text) if c == 10]
    start = ends[-3] + 1
    jobs = [(0, 0, 0, None, text[:n]) for n in range(start, len(text) + 1)]
    check(jobs, [f"cut{n}" for n in range(start, len(text) + 1)])
    for (flags, head, ref_len, rname, t), got in zip(jobs, run(jobs)):
        full = sum(1 for i in ends if i < len(t))
        rows = [r for r in t[:ends[full - 1] + 1].split(b"\n")[:-1]]
        assert got["info"][0] == sum(1 for r in rows if not r.startswith(b"@")) and got["info"][5] == ends[full - 1] + 1


def test_model_under_the_host_sanitizers():
    jobs = [(flags, head, 3, rname, text) for _, text in sc.CASES for flags, head, rname in ((sc.FINAL, 0, None), (0, 5, b"chr"), (sc.FINAL | sc.QUAL_FORWARD, 15, b"chr"))]
    check(jobs, [n for n, _ in sc.CASES for _ in range(3)], sanitize=True)


def test_the_symbol_is_in_every_list():
    from zoe_amd import _lib

    name = "zsw_sam_parse_batch"
    assert name in _lib.SYMBOLS
    for rel in (("include", "zoe_sw.h"), ("bindings", "rust", "zoe_sw_gpu.rs"), ("examples", "zsw_c_abi.c"), ("zoe_amd", "records.py"), ("zoe_amd", "alignment.py"),
                ("INTEGRATION.md",), ("DESIGN.md",), ("README.md",)):
        assert name in open(os.path.join(ROOT, *rel)).read(), rel
    assert "zsw_samtext.hip" in open(os.path.join(ROOT, "zoe_amd", "build.py")).read()
    assert "zsw_*" in open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_exports.map")).read()
    h = open(os.path.join(ROOT, "include", "zoe_sw.h")).read()
    for k, word in enumerate(sc.INFO):
        assert re.search(r"ZSW_SAMTEXT_INFO_" + word.upper() + r" = " + str(k) + r"\b", h), word
        assert getattr(_lib, "SAMTEXT_INFO_" + word.upper()) == k
    assert re.search(r"ZSW_SAMTEXT_INFO_WORDS = 13\b", h) and _lib.SAMTEXT_INFO_WORDS == 13
    assert (sc.FINAL, sc.QUAL_FORWARD) == (_lib.SAMTEXT_FINAL, _lib.SAMTEXT_QUAL_FORWARD)
    for prefix, names in (("SAMTEXT_", ("INVALID_UTF8", "TOO_FEW_FIELDS", "INVALID_FLAG", "INVALID_POS", "INVALID_MAPQ", "INVALID_QUALITY")),
                          ("SAMREC_", ("SEQ_MISSING", "CIGAR_INVALID_OP", "CIGAR_MISSING_INC", "CIGAR_INC_ZERO", "CIGAR_INC_OVERFLOW", "CIGAR_MISSING_OP",
                                       "CIGAR_MERGE_OVERFLOW", "POS_ZERO", "CLIPS_EXCEED_SEQ", "TOO_LARGE"))):
        for k, word in enumerate(names, 1):
            assert re.search(r"ZSW_" + prefix + word + r" = " + str(k) + r"\b", h), word
            assert getattr(_lib, prefix + word) == k == getattr(sc, word)
    for k, word in enumerate(("NO_SCORE", "OTHER_RNAME", "SEQ_MISSING", "QUAL_MISSING", "QUAL_LENGTH")):
        assert re.search(r"ZSW_SAMREC_BIT_" + word + r" = " + str(1 << k) + r"\b", h) and getattr(_lib, "SAMREC_BIT_" + word) == 1 << k == getattr(sc, "BIT_" + word)
    rs = open(os.path.join(ROOT, "bindings", "rust", "zoe_sw_gpu.rs")).read()
    assert "pub struct ZswSamParsed" in rs and "pub struct ZswSamParseOut" in rs and len(re.findall(r"\b" + name + r"\(", rs)) >= 2
