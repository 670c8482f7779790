"""CPU checks of zsw_sam_batch (no GPU): the host model tests/models/sam_line.cpp — zoe_amd/csrc/zsw_sam.hpp, the text the kernel
compiles, behind a loop over the lanes — against tests/sam_ref.py on the shape list of tests/sam_cases.py; sam_ref.py itself against
SamData of zoe_amd/records.py; the malformed records once more through an -fsanitize=address,undefined build of the model; and the
symbol in every list. The model itself requires line_length() == the bytes write_line() puts, every byte put exactly once."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sam_cases as sc
import sam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_sam.hpp")

_built = {}


def header_constant(name: str) -> int:
    return int(re.search(r"constexpr \w+ " + name + r" = (\d+);", open(HEADER).read()).group(1))


def model(sanitize: bool = False) -> str:
    if sanitize not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_sam_"), "sam_line" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "models", "sam_line.cpp")], check=True)
        _built[sanitize] = exe
    return _built[sanitize]


def run(lines, sanitize=False):
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.run([model(sanitize), f.name], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
    return out.stdout.splitlines()


def hx(b) -> str:
    return bytes(b).hex() or "-"


def case_line(c, rec, inc, op, cfg, mapq=255, rname=sc.RNAME):
    names, quals, strand, stats, omit = cfg
    m = c["stats"]
    return (f"case {1 if omit else 0} {c['status']} {int(names)} {hx(c['name'])} {int(quals)} {hx(c['qual'])} {hx(c['read'])} {c['strand'] if strand else -1} "
            f"{int(stats)} {m[0]} {m[1]} {m[2]} {hx(rname)} {mapq} {rec['score']} {rec['ref_start']} {rec['n_ciglets']} {rec['ciglet_offset']} {len(inc)} "
            + " ".join(f"{int(i)} {int(o)}" for i, o in zip(inc, op)))


def check(cases, cfg, sanitize=False):
    """every case alone (its own ciglet arrays) through the model; -> how many it reports as malformed"""
    lines, want = [], []
    for c in cases:
        recs, inc, op = sc.assemble([c])
        lines.append(case_line(c, recs[0], inc, op, cfg))
        want.append(sc.line_of(c, recs[0], inc, op, cfg))
    got = run(lines, sanitize)
    assert len(got) == len(cases)
    for c, g, (text, bad) in zip(cases, got, want):
        g_bad, g_len, g_hex = (g.split(" ") + [""])[:3]
        assert (int(g_bad), int(g_len), bytes.fromhex(g_hex)) == (int(bad), len(text), text), (c["name"], cfg)
    return sum(bad for _, bad in want)


def test_header_constants():
    assert header_constant("SAM_G") == 64
    assert header_constant("SAM_BLOCK_LINES") >= 1 and header_constant("SAM_LDS_LINE") >= 256


def test_dec_digits_and_the_decimal_writer():
    got = run([f"dec {v}" for v in sc.DEC_VALUES])
    assert got == [f"{len(str(v))} {v}" for v in sc.DEC_VALUES]
    assert {0, 9, 10, 99, 100, 2 ** 32 - 1, 2 ** 32, 3 * (2 ** 32 - 1)} <= set(sc.DEC_VALUES)


@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=lambda c: "".join("NQSTO"[k] if on else "-" for k, on in enumerate(c)))
def test_model_equals_reference_on_the_shape_list(cfg):
    cap = header_constant("SAM_LDS_LINE")
    cases = sc.shape_cases(cap, cfg)
    n_bad = check(cases, cfg)
    assert n_bad == sum(c["name"].startswith(b"bad_") for c in cases) == 9
    if cfg == sc.CONFIGS[0]:  # the list holds what it claims to: lines one byte each side of the LDS cap, every sweep edge
        lens = set()
        for c in cases:
            recs, inc, op = sc.assemble([c])
            lens.add(len(sc.line_of(c, recs[0], inc, op, cfg)[0]))
        assert {cap - 1, cap, cap + 1} <= lens
        assert {len(c["cig"]) for c in cases} >= {0, 1, 63, 64, 65, 3000}
        assert {len(c["name"]) for c in cases} >= set(range(32))
        assert {len(c["read"]) for c in cases} >= {0, 1, 63, 64, 65}
        assert {c["status"] for c in cases} >= {0, 1, 2, 3, 4}


def test_known_lines():
    """written out by hand: the two shapes, the 64-bit sums, `*` for what is missing"""
    rec = {"score": 300, "ref_start": 2 ** 32 - 1, "n_ciglets": 2, "ciglet_offset": 1}
    inc, op = np.array([7, 100, 5], dtype=np.uint32), np.frombuffer(b"SM=", dtype=np.uint8)
    u = 2 ** 32 - 1
    assert sam_ref.sam_line(b"r1", b"ACG", b"!#%", 0, rec, inc, op, b"chr", 60, 1, (u, u, u)) == (
        b"r1\t16\tchr\t4294967296\t60\t100M5=\t*\t0\t0\tACG\t%#!\tAS:i:300\tNM:i:12884901885\n", False)
    assert sam_ref.sam_line(None, b"", None, 0, dict(rec, n_ciglets=0), inc, op, b"chr") == (b"*\t0\tchr\t4294967296\t255\t*\t*\t0\t0\t*\t*\tAS:i:300\n", False)
    assert sam_ref.sam_line(b"r2", b"AC", b"!#", 4, rec, inc, op, b"chr", 60, 1, (1, 1, 1)) == (b"r2\t4\t*\t0\t0\t*\t*\t0\t0\tAC\t#!\n", False)
    assert sam_ref.sam_line(b"r3", b"AC", b"!#", 0, dict(rec, ciglet_offset=2), inc, op, b"chr", omit_seq=True) == (b"r3\t4\t*\t0\t0\t*\t*\t0\t0\t*\t!#\n", True)
    c = sc.case(b"r1", read=b"ACG", strand=1, stats=(u, u, u), score=300, ref_start=u, cig=[(100, ord("M")), (5, ord("="))])
    c["qual"] = b"!#%"
    recs, inc2, op2 = sc.assemble([c])
    got = run([case_line(c, recs[0], inc2, op2, sc.CONFIGS[0], mapq=60, rname=b"chr")])
    assert bytes.fromhex(got[0].split(" ")[2]) == b"r1\t16\tchr\t4294967296\t60\t100M5=\t*\t0\t0\tACG\t%#!\tAS:i:300\tNM:i:12884901885\n"


def test_reference_agrees_with_samdata():
    """sam_ref.py against str(SamData.from_alignment(..)) / SamData.unmapped(..) of zoe_amd/records.py on what both can express:
    well-formed records with at least one ciglet, names that are text, forward strand"""
    from zoe_amd.alignment import ALN_DTYPE, STATS_DTYPE, AlignmentBatch
    from zoe_amd.records import SamData

    cases = [c for c in sc.shape_cases(header_constant("SAM_LDS_LINE")) if not c["name"].startswith(b"bad_") and (c["cig"] or c["status"] != 0)]
    recs, inc, op = sc.assemble(cases)
    records = np.zeros(len(cases), dtype=ALN_DTYPE)
    stats = np.zeros(len(cases), dtype=STATS_DTYPE)
    for k, (c, r) in enumerate(zip(cases, recs)):
        for key in ("score", "ref_start", "n_ciglets", "ciglet_offset"):
            records[k][key] = r[key]
        stats[k]["mismatches"], stats[k]["ins_bases"], stats[k]["del_bases"] = (min(v, 2 ** 30) for v in c["stats"])  # numpy adds in 32 bits
    aln = AlignmentBatch(np.array([c["status"] for c in cases], dtype=np.uint8), records, inc, op)
    n = 0
    for k, (c, r) in enumerate(zip(cases, recs)):
        for with_stats in (False, True):
            st = tuple(int(stats[k][f]) for f in ("mismatches", "ins_bases", "del_bases")) if with_stats else None
            want, bad = sam_ref.sam_line(c["name"], c["read"], c["qual"], c["status"], r, inc, op, b"ref1", 255, 0, st)
            assert not bad
            if c["status"] == 0:
                rec = SamData.from_alignment(aln, k, c["name"].decode(), 0, "ref1", 255, c["read"], c["qual"], stats if with_stats else None)
            else:
                rec = SamData.unmapped(c["name"].decode(), c["read"], c["qual"])
            assert (str(rec) + "\n").encode() == want, c["name"]
            n += 1
    assert n > 100


def test_malformed_records_under_the_sanitizers():
    """the malformed records, every array in a heap block of its exact size, through the -fsanitize=address,undefined build of the
    stand-alone model: no index derived from a record leaves its array"""
    for cfg in (sc.CONFIGS[0], sc.CONFIGS[-1]):
        assert check(sc.malformed_cases(), cfg, sanitize=True) == 9


def test_the_symbol_is_in_every_list():
    from zoe_amd import _lib

    assert "zsw_sam_batch" in _lib.SYMBOLS
    for rel in (("include", "zoe_sw.h"), ("examples", "zsw_c_abi.c"), ("bindings", "rust", "zoe_sw_gpu.rs"), ("INTEGRATION.md",)):
        assert "zsw_sam_batch" in open(os.path.join(ROOT, *rel)).read(), rel
    assert "zsw_sam.hip" in open(os.path.join(ROOT, "zoe_amd", "build.py")).read()
