"""CPU checks of zsw_pileup_batch / zsw_consensus_from_counts (no GPU): the host model tests/models/pileup_walk.cpp —
zoe_amd/csrc/zsw_pileup.hpp, the text the kernels compile, behind a loop over the lanes — against tests/pileup_ref.py: the bin of
every byte, the reference's known answers for plurality_acgtn, oracle alignments in both roles and both `invert` values,
hand-built records for every op and every way to be malformed, the malformed ones once more through an
-fsanitize=address,undefined build of the model, and the symbols in every list."""
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import annotate_ref as ar
import pileup_ref as pr
from conftest import stable_seed
from test_annotate_model import READ, ROLES, SEQ, case_cigar, status_cases, sweep_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64  # zsw_pileup.hpp: PILEUP_G

_built = {}


def model(sanitize: bool = False) -> str:
    if sanitize not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_pileup_"), "pileup_walk" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "models", "pileup_walk.cpp")], check=True)
        _built[sanitize] = exe
    return _built[sanitize]


def run_lines(lines, sanitize=False):
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.run([model(sanitize), f.name], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
    return out.stdout.splitlines()


def case_line(c):
    r = c["rec"]
    return (f"case {c['flags']} {c['status']} {c['read'].hex() or '-'} {r['score']} {r['ref_start']} {r['ref_end']} {r['query_start']} {r['query_end']} "
            f"{r['ref_len']} {r['query_len']} {r['n_ciglets']} {r['ciglet_offset']} {len(c['inc'])} " + " ".join(f"{i} {o}" for i, o in zip(c["inc"], c["op"])))


def run_model(cases, sanitize=False):
    """cases that share seq and the role bit -> (counts (len, 8), ins (len + 1, 2), n_bad) of the one table they pile up to"""
    seq = cases[0]["seq"]
    assert all(c["seq"] == seq for c in cases)
    out = run_lines(["seq " + (seq.hex() or "-")] + [case_line(c) for c in cases] + ["table"], sanitize)
    L = len(seq)
    assert len(out) == 1 + L + L + 1
    counts = np.array([[int(x) for x in line.split()] for line in out[1:1 + L]], dtype=np.uint32).reshape(L, 8)
    ins = np.array([[int(x) for x in line.split()] for line in out[1 + L:]], dtype=np.uint32).reshape(L + 1, 2)
    return counts, ins, int(out[0])


def want_of(cases):
    """pileup_ref over the same cases, each with ciglet arrays of its own"""
    seq, flags = cases[0]["seq"], cases[0]["flags"]
    counts, ins, n_bad = None, None, 0
    for c in cases:
        assert c["flags"] == flags
        counts, ins, bad = pr.pileup([c["rec"]], [c["status"]], c["inc"], c["op"], [c["read"]], seq, flags, counts, ins)
        n_bad += bad
    return counts, ins, n_bad


def check(cases, sanitize=False):
    got, want = run_model(cases, sanitize), want_of(cases)
    assert got[2] == want[2], (got[2], want[2])
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), (bad[:5], got[0][bad[0][0]], want[0][bad[0][0]])
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    return got


def test_header_constants():
    txt = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_pileup.hpp")).read()
    assert re.search(r"constexpr int PILEUP_G = (\d+);", txt).group(1) == str(G)
    lds = int(re.search(r"constexpr uint32_t PILEUP_LDS_SITES_MAX = (\d+);", txt).group(1))
    assert 2000 <= lds < 30000  # a 2 kb reference accumulates in LDS; 16 bytes per site: 30 kb cannot


# ---- the bins and the vote -------------------------------------------------------------------------------------------------------

def test_the_bin_of_every_byte():
    """the table as the issue spells it, byte by byte, against both implementations"""
    want = [7] * 256
    for chars, b in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3), ("Nn", 4), ("-", 5), ("RYSWKMBDHVryswkmbdhv.", 6)):
        for ch in chars:
            want[ord(ch)] = b
    assert [pr.bin_of(b) for b in range(256)] == want
    assert [int(x) for x in run_lines(["bins " + bytes(range(256)).hex()])[0].split()] == want
    assert sum(1 for x in want if x != 7) == 34


def known_answers():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "plurality_known_answers.json")))["cases"]


def test_plurality_known_answers():
    cases = known_answers()
    assert len(cases) == 9
    got = run_lines([f"plurality {c['input'].encode().hex() or '-'}" for c in cases])
    for c, g in zip(cases, got):
        assert chr(pr.plurality_acgtn(pr.composition(c["input"].encode()))) == c["expected"], c
        assert chr(int(g)) == c["expected"], c


def tie_table():
    """every subset of A C G T N tied at the top, above and below the others; the gap, other and invalid bins larger than any"""
    rows = []
    for mask in range(32):
        rows.append([5 if mask >> b & 1 else 2 for b in range(5)] + [9, 9, 9])
        rows.append([5 if mask >> b & 1 else 0 for b in range(5)] + [0, 0, 0])
    rows.append([0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0xFFFFFFFE, 0, 0, 0])
    rows.append([0x80000000, 0, 0, 0, 0x80000000, 0, 0, 0])  # the five bins sum to 0 modulo 2^32: covered all the same
    return rows


def test_consensus_ties_and_uncovered_sites():
    rows = tie_table()
    fb = bytes((b"acgtn-RY#" * 20)[:len(rows)])
    for flags in (0, pr.KEEP_UNCOVERED):
        got = run_lines([f"consensus {flags} {fb.hex() if flags else '-'} {len(rows)}"] + [" ".join(map(str, r)) for r in rows])
        got = bytes(int(x) for x in got[0].split())
        assert got == pr.consensus(rows, flags, fb)
        for r, g, f in zip(rows, got, fb):
            if flags and not any(r[:5]):
                assert g == f
            else:
                assert g == b"ACGTN"[min(b for b in range(5) if r[b] == max(r[:5]))]
    assert pr.consensus([[0] * 8, [0, 0, 0, 0, 0, 7, 7, 7]], 0) == b"AA"


# ---- known answer ----------------------------------------------------------------------------------------------------------------

DOC_REF, DOC_QUERY = b"ATGCATCGATCGATCGATCGATCGATCGATGC", b"CGTTCGCCATAAAGGGGG"


def test_known_answer_of_the_doc_example():
    """striped.rs:418-441: ref 14..31, query 0..15, 6M2D9M3S. By hand: CGATCG|AT|CGATCGATG over CGTTCG|--|CCATAAAGG, so positions
    14..19 see C G T T C G, 20..21 a gap, 22..30 C C A T A A A G G; and with the roles swapped the same columns pile up on the other
    sequence: positions 0..5 of CGTTCG... see C G A T C G, an insertion of 2 in front of 6, positions 6..14 see C G A T C G A T G"""
    fwd = case_cigar(0, DOC_QUERY, DOC_REF, 26, (14, 31), (0, 15), "6M2D9M3S")
    counts, ins, bad = check([fwd])
    assert bad == 0 and not ins.any()
    seen = {14 + k: pr.bin_of(b) for k, b in enumerate(b"CGTTCG--CCATAAAGG")}
    for pos in range(len(DOC_REF)):
        want = [0] * 8
        if pos in seen:
            want[seen[pos]] = 1
        assert counts[pos].tolist() == want, pos
    inv = case_cigar(ar.READ_IS_REF, DOC_REF, DOC_QUERY, 26, (14, 31), (0, 15), "6M2D9M3S")  # the same record: the table is over DOC_QUERY
    counts, ins, bad = check([inv])
    assert bad == 0
    seen = {k: pr.bin_of(b) for k, b in enumerate(b"CGATCG" + b"CGATCGATG")}
    for pos in range(len(DOC_QUERY)):
        want = [0] * 8
        if pos in seen:
            want[seen[pos]] = 1
        assert counts[pos].tolist() == want, pos
    assert ins[6].tolist() == [1, 2] and ins.sum() == 3


# ---- model == pileup_ref on oracle alignments ---------------------------------------------------------------------------------------

def oracle_tables(oracle, sc, pairs, T="i16", lanes=16):
    """(read, seq) pairs that share seq, through oracle.align in both roles and both invert values -> one checked table per role"""
    n = 0
    for shared, invert, flags in ROLES:
        cases = []
        for read, seq in pairs:
            a = oracle.align(T, lanes, sc, seq if shared else read, read if shared else seq, other_is_query=bool(invert))
            if a.status == 0:
                cases.append(case_cigar(flags, read, seq, a.score, a.ref_range, a.query_range, a.cigar))
        assert cases
        counts, ins, bad = check(cases)
        assert bad == 0
        # every column of every alignment is somewhere: columns + gaps on the sequence = the sequence's range of each record
        span = sum((c["rec"]["query_end"] - c["rec"]["query_start"]) if flags & ar.READ_IS_REF else (c["rec"]["ref_end"] - c["rec"]["ref_start"]) for c in cases)
        assert int(counts.sum()) == span, (flags, counts.sum(), span)
        n += len(cases)
    return n


@pytest.mark.parametrize("scheme", [(2, -5, -10, -1), (4, -2, -3, -1)])
def test_random_pairs(oracle, scheme):
    ma, mi, go, ge = scheme
    rng = np.random.default_rng(stable_seed("pileup", scheme))
    sc = oracle.dna_scoring(ma, mi, b"N", go, ge)
    alpha = np.frombuffer(b"ACGTNacgtURy-#", dtype=np.uint8)
    ref = bytearray(rng.choice(alpha[:4], 400))
    for k in rng.integers(0, 400, 40):
        ref[k] = int(rng.choice(alpha))  # lower case, N, U, IUPAC, a gap and an invalid byte in the sequence itself
    ref = bytes(ref)
    pairs = []
    for _ in range(80):
        L = int(rng.integers(8, 200))
        s = int(rng.integers(0, 400 - L))
        r = bytearray(ref[s:s + L])
        for _ in range(int(rng.integers(0, 7))):
            k = int(rng.integers(0, max(1, len(r))))
            t = rng.random()
            if t < 0.4:
                r[k] = int(rng.choice(alpha))
            elif t < 0.7:
                del r[k:k + int(rng.integers(1, 4))]
            else:
                r[k:k] = bytes(rng.choice(alpha[:4], int(rng.integers(1, 4))))
        pairs.append((bytes(r) or b"A", ref))
    assert oracle_tables(oracle, sc, pairs) >= 200


def test_h5_against_h1_lower_case_against_upper_case(oracle, h5, h1):
    """NC_026433.1 is lower-case, NC_007362.1 upper-case: a lower-case base of the sequence is "as expected" for the upper-case base
    of the read, since both fall in one bin — the cover route carries the matching columns although no byte is equal"""
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    assert h1[:40].islower() and h5[:40].isupper()
    assert oracle_tables(oracle, sc, [(h5, h1)]) == 4


# ---- every op, every way to be malformed, hand-built --------------------------------------------------------------------------------

def op_cases():
    """flags 0 over SEQ unless said; every op, runs on both sides of a sweep, a run that starts at 0 and one that ends at len"""
    L = len(SEQ)
    out = [
        case_cigar(0, READ, SEQ, 0, (20, 120), (0, 100), "100M"),
        case_cigar(0, READ, SEQ, 0, (20, 120), (0, 100), "5H2P40=1X59=3H"),
        case_cigar(0, SEQ[20:30] + b"TTTTT" + SEQ[35:120], SEQ, 0, (20, 120), (0, 100), "10M5N5S85M"),
        case_cigar(0, SEQ[20:70] + SEQ[75:125], SEQ, 0, (20, 125), (0, 100), "50M5D50M"),
        case_cigar(0, SEQ[20:70] + b"GG" + b"T" + SEQ[70:117], SEQ, 0, (20, 117), (0, 100), "50M2I1I47M"),  # two runs in front of one position
        case_cigar(0, b"TT" + SEQ[:98], SEQ, 0, (0, 98), (0, 100), "2I98M"),                                  # an insertion in front of position 0
        case_cigar(0, SEQ[L - 98:] + b"TT", SEQ, 0, (L - 98, L), (0, 100), "98M2I"),                          # ... and in front of len
        case_cigar(0, SEQ, SEQ, 0, (0, L), (0, L), f"{L}M"),                                                  # from 0 to the last position
        case_cigar(0, SEQ[:10], SEQ, 0, (0, L), (0, 10), f"10M{L - 10}D"),                                    # a gap range that ends at len
        case_cigar(0, SEQ[:10], SEQ, 0, (0, L), (0, 10), f"{L - 10}N10M"),                                    # an N range that starts at 0
        case_cigar(0, READ, SEQ, 0, (20, 120), (0, 100), "100M", status=2),                                   # not SOME: neither counted nor bad
        case_cigar(0, b"", SEQ, 0, (20, 20), (0, 0), ""),                                                     # no ciglets: nothing, and not bad
    ]
    other = bytes(b"ACGT"[(b"ACGT".index(b) + 1) % 4] for b in READ)
    out.append(case_cigar(0, other, SEQ, 0, (20, 120), (0, 100), "100M"))                                     # every column a miss
    out.append(case_cigar(0, bytes(o if k & 1 else b for k, (b, o) in enumerate(zip(READ, other))), SEQ, 0, (20, 120), (0, 100), "1=1X" * 50))
    out.append(case_cigar(0, READ.lower().replace(b"t", b"u"), SEQ, 0, (20, 120), (0, 100), "100M"))          # lower case and U: as expected
    out.append(case_cigar(0, b"RYSWKMBDHVryswkmbdhv.-#@\x00\xff" + READ[26:], SEQ, 0, (20, 120), (0, 100), "100M"))
    ins = bytes(b for k in range(35) for b in (READ[k], ord("T")))
    out.append(case_cigar(0, ins + READ[35:], SEQ, 0, (20, 120), (0, 135), "1M1I" * 35 + "65M"))              # 71 ciglets
    return out


def swap_cases():
    """READ_IS_REF: the record's reference is the read, its query SEQ"""
    L = len(SEQ)
    f = ar.READ_IS_REF
    return [
        case_cigar(f, READ, SEQ, 0, (0, 100), (20, 120), f"20S100M{L - 120}S"),
        case_cigar(f, READ[:50] + READ[55:], SEQ, 0, (0, 95), (20, 120), f"20S50M5I45M{L - 120}S"),           # I: positions of SEQ opposite nothing
        case_cigar(f, READ[:50] + b"GGG" + READ[50:], SEQ, 0, (0, 103), (20, 120), f"20S50M3D50M{L - 120}S"),  # D: read bases opposite nothing
        case_cigar(f, READ[:50] + b"GGG" + READ[50:], SEQ, 0, (0, 103), (20, 120), f"20S50M3N50M{L - 120}S"),  # N: nothing, the read moves on
        case_cigar(f, b"GG" + READ, SEQ, 0, (2, 102), (20, 120), f"20S100M{L - 120}S"),                        # ref_start into the read
        case_cigar(f, READ, SEQ, 0, (0, 100), (20, 120), f"20S100M{L - 120}S", status=1),
        case_cigar(f, READ, SEQ, 0, (0, 100), (20, 120), f"20S101M{L - 121}S"),                                # leaves the read
        case_cigar(f, READ, SEQ, 0, (0, 100), (20, 120), f"20S100M{L - 119}S"),                                # leaves SEQ
        case_cigar(f, SEQ[L - 5:], SEQ, 0, (0, 5), (L - 5, L), f"{L - 5}S5M"),                                 # ends on the last position
        case_cigar(f, SEQ[L - 5:] + b"T", SEQ, 0, (0, 6), (L - 5, L), f"{L - 5}S5M1D"),                        # an insertion in front of len
    ]


def malformed_cases():
    """the hand-built records of the annotate model (every ZSW_PATH_* status): here a record either counts or is one of n_bad"""
    return [c for _, c in status_cases() if c["flags"] == 0]


def test_every_op(oracle):
    counts, ins, bad = check(op_cases())
    assert bad == 0 and ins.sum() > 0
    assert counts[:, pr.GAP].sum() == 5 + len(SEQ) - 10 + 1 and counts[:, pr.N].sum() == 5 + len(SEQ) - 10  # + 1: the `-` byte of a read
    assert counts[:, pr.OTHER].sum() == 21 and counts[:, pr.INVALID].sum() == 4 and ins[0].tolist() == [1, 2] and ins[len(SEQ)].tolist() == [1, 2]
    assert ins[70].tolist() == [2, 3]


def test_the_role_swap():
    counts, ins, bad = check(swap_cases())
    assert bad == 2 and counts[:, pr.GAP].sum() == 5 and counts[:, pr.N].sum() == 0 and ins[70].tolist() == [1, 3] and ins[len(SEQ)].tolist() == [1, 1]
    assert not counts[:20].any()  # S skips positions of the sequence without counting them


def test_malformed_records_count_and_contribute_nothing():
    cases = malformed_cases()
    want_bad = 0
    for st, c in status_cases():
        if c["flags"] != 0:
            continue
        one = run_model([c])
        good = st in ar.ANNOTATED or (st == ar.BAD_RECORD and ar.cigar_string(zip(c["inc"], c["op"])).startswith("4294967295H"))  # nothing is merged here
        if st == ar.NO_ALIGNMENT:
            assert one[2] == 0 and not one[0].any() and not one[1].any()
        elif good:
            assert one[2] == 0 and one[0].any(), (st, ar.cigar_string(zip(c["inc"], c["op"])))
        else:
            assert one[2] == 1 and not one[0].any() and not one[1].any(), (st, ar.cigar_string(zip(c["inc"], c["op"])))
            want_bad += 1
    assert want_bad >= 20
    assert check(cases)[2] == want_bad


def test_sweep_boundaries():
    """M runs of 1, G, G + 1 and 2G + 3 columns with a mismatch on each side of every sweep boundary"""
    by_seq = {}
    for c in sweep_cases():
        by_seq.setdefault(c["seq"], []).append(c)
    for cases in by_seq.values():
        assert check(cases)[2] == 0


def test_malformed_records_under_sanitizers():
    """the model built with -fsanitize=address,undefined (a stand-alone executable, nothing preloaded) over the hand-built records:
    every array in a heap block of exactly its size, so an index that leaves one ends the run"""
    check(malformed_cases() + op_cases(), sanitize=True)
    check(swap_cases(), sanitize=True)
    by_seq = {}
    for c in sweep_cases():
        by_seq.setdefault(c["seq"], []).append(c)
    for cases in by_seq.values():
        check(cases, sanitize=True)


def test_the_symbols_are_in_every_list():
    from zoe_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zoe_sw.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "zoe_sw_gpu.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "zoe_sw.hpp")).read()
    for name in ("zsw_pileup_batch", "zsw_consensus_from_counts"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SYMBOLS
        assert len(re.findall(r"\b" + name + r"\(", rs)) >= 2 and name in hpp
        assert name in open(os.path.join(ROOT, "examples", "zsw_c_abi.c")).read() and name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "zsw_site_counts" in hdr and "zsw_site_insertions" in hdr and "pub struct ZswSiteCounts" in rs
    assert re.search(r"ZSW_PILEUP_CLEAR\s*=\s*8\b", hdr) and _lib.PILEUP_CLEAR == pr.CLEAR == 8 and "ZSW_PILEUP_CLEAR: i32 = 8" in rs
    assert re.search(r"ZSW_CONSENSUS_KEEP_UNCOVERED\s*=\s*1\b", hdr) and _lib.CONSENSUS_KEEP_UNCOVERED == pr.KEEP_UNCOVERED == 1
    assert (pr.READ_IS_REF, pr.SHARED) == (_lib.ANNOTATE_READ_IS_REF, _lib.ANNOTATE_SHARED)
    assert "zsw_*" in open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_exports.map")).read()
