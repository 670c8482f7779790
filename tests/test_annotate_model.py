"""CPU checks of zsw_annotate_batch (no GPU): the host model tests/models/annotate_walk.cpp — zoe_amd/csrc/zsw_annotate.hpp, the
text the kernel compiles, behind a loop over the lanes — against tests/annotate_ref.py: a known answer derived by hand, oracle
alignments in both roles and both `invert` values under both equalities, hand-built records for every ZSW_PATH_* status, the
malformed ones once more through an -fsanitize=address,undefined build of the model, and the symbol in every list."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import annotate_ref as ar
from conftest import stable_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64  # zsw_annotate.hpp: ANN_G

_built = {}


def model(sanitize: bool = False) -> str:
    if sanitize not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_annotate_"), "annotate_walk" + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "models", "annotate_walk.cpp")], check=True)
        _built[sanitize] = exe
    return _built[sanitize]


def test_header_constants():
    txt = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_annotate.hpp")).read()
    assert re.search(r"constexpr int ANN_G = (\d+);", txt).group(1) == str(G)


# ---- cases ---------------------------------------------------------------------------------------------------------------------

def rec_of(score, rr, qr, ref_len, query_len, n, off=0):
    return {"score": score, "ref_start": rr[0], "ref_end": rr[1], "query_start": qr[0], "query_end": qr[1], "ref_len": ref_len,
            "query_len": query_len, "n_ciglets": n, "ciglet_offset": off}


def case_of(flags, read, seq, rec, cig, status=0):
    """cig: the call's whole ciglet arrays as [(inc, op)]"""
    return {"flags": flags, "status": status, "read": bytes(read), "seq": bytes(seq), "rec": rec, "inc": [c[0] for c in cig], "op": [c[1] for c in cig]}


def case_cigar(flags, read, seq, score, rr, qr, cigar, status=0):
    """a record over exactly its own ciglets; lengths taken from the sequences the flags give the two roles"""
    cig = ar.parse_cigar(cigar)
    reference, query = (read, seq) if flags & ar.READ_IS_REF else (seq, read)
    return case_of(flags, read, seq, rec_of(score, rr, qr, len(reference), len(query), len(cig)), cig, status)


def run_model(sc, cases, sanitize=False):
    """-> [(stats tuple of 8, verbose ciglets)] per case"""
    lines = [f"scoring {sc.S} {-sc.gap_open} {-sc.gap_extend}", " ".join(str(int(x)) for x in sc.index_map),
             " ".join(str(int(x)) for x in np.asarray(sc.weights).reshape(-1))]
    seq = None
    for c in cases:
        if c["seq"] != seq:
            seq = c["seq"]
            lines.append("seq " + (seq.hex() or "-"))
        r = c["rec"]
        lines.append(f"case {c['flags']} {c['status']} {c['read'].hex() or '-'} {r['score']} {r['ref_start']} {r['ref_end']} {r['query_start']} {r['query_end']} "
                     f"{r['ref_len']} {r['query_len']} {r['n_ciglets']} {r['ciglet_offset']} {len(c['inc'])} " + " ".join(f"{i} {o}" for i, o in zip(c["inc"], c["op"])))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.run([model(sanitize), f.name], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
    res = []
    for line in out.stdout.splitlines():
        v = [int(x) for x in line.split()]
        res.append((tuple(v[:8]), [(v[9 + 2 * k], v[10 + 2 * k]) for k in range(v[8])]))
    assert len(res) == len(cases)
    return res


def want_of(sc, c):
    return ar.annotate_record(c["rec"], c["status"], c["inc"], c["op"], c["read"], c["seq"], c["flags"], sc.weights, sc.index_map, sc.gap_open, sc.gap_extend)


def check(sc, cases, sanitize=False):
    got = run_model(sc, cases, sanitize)
    for k, (c, g) in enumerate(zip(cases, got)):
        w = want_of(sc, c)
        assert g == (tuple(w[0]), list(w[1])), (k, c["flags"], ar.cigar_string(zip(c["inc"], c["op"])), g, w)
    return got


# ---- known answer --------------------------------------------------------------------------------------------------------------

DOC_REF, DOC_QUERY = b"ATGCATCGATCGATCGATCGATCGATCGATGC", b"CGTTCGCCATAAAGGGGG"


def test_known_answer_of_the_doc_example(oracle):
    """striped.rs:418-441: ref 14..31, query 0..15, 6M2D9M3S, score 26 at 4 / -2, gaps -3 / -1. By hand, column by column:
    GATCGA|TC|GATCGATGC under CGTTCG|--|CCATAAAGG: == X === DD = X == XX = X =."""
    sc = oracle.dna_scoring(4, -2, b"N", -3, -1)
    fwd = case_cigar(0, DOC_QUERY, DOC_REF, 26, (14, 31), (0, 15), "6M2D9M3S")
    inv = case_cigar(ar.READ_IS_REF, DOC_QUERY, DOC_REF, 26, (0, 15), (14, 31), "14S6M2I9M1S")  # Alignment::invert of the record
    got = run_model(sc, [fwd, inv])
    assert got[0][0] == (10, 5, 0, 2, 0, 1, 26, ar.OK) and ar.cigar_string(got[0][1]) == "2=1X3=2D1=1X2=2X1=1X1=3S"
    assert got[1][0] == (10, 5, 2, 0, 1, 0, 26, ar.OK) and ar.cigar_string(got[1][1]) == "14S2=1X3=2I1=1X2=2X1=1X1=1S"
    for c, g in zip((fwd, inv), got):
        w = want_of(sc, c)
        assert (tuple(w[0]), w[1]) == g


# ---- model == annotate_ref on oracle alignments -----------------------------------------------------------------------------------

ROLES = ((False, 0, 0), (False, 1, ar.READ_IS_REF), (True, 0, ar.SHARED | ar.READ_IS_REF), (True, 1, ar.SHARED))  # shared, invert, flags


def oracle_cases(oracle, sc, pairs, T="i16", lanes=16):
    """(read, seq) pairs through oracle.align in both roles and both invert values; both equalities"""
    cases, alns = [], []
    for read, seq in pairs:
        for shared, invert, flags in ROLES:
            a = oracle.align(T, lanes, sc, seq if shared else read, read if shared else seq, other_is_query=bool(invert))
            if a.status != 0:
                continue
            for eq in (0, ar.MATCH_RESIDUES):
                cases.append(case_cigar(flags | eq, read, seq, a.score, a.ref_range, a.query_range, a.cigar))
                alns.append((a, invert))
    return cases, alns


def check_oracle_cases(oracle, sc, pairs, **kw):
    cases, alns = oracle_cases(oracle, sc, pairs, **kw)
    assert cases
    got = check(sc, cases)
    for c, (a, invert), (stats, verbose) in zip(cases, alns, got):
        assert stats[7] == ar.OK and stats[6] == a.score, (a, stats)  # the self-check of every CIGAR
        reference, query = (c["read"], c["seq"]) if c["flags"] & ar.READ_IS_REF else (c["seq"], c["read"])
        if not invert:  # the record's query is the profile sequence: the oracle's own sw_score_from_path applies as it stands
            assert oracle.score_from_path(sc, query, reference[a.ref_range[0]:a.ref_range[1]], a.cigar) == a.score
        assert stats[0] + stats[1] + stats[2] == a.query_range[1] - a.query_range[0]
        assert stats[0] + stats[1] + stats[3] == a.ref_range[1] - a.ref_range[0]
        folded = []
        for inc, op in verbose:
            ar.add_ciglet(folded, inc, ord("M") if op in b"=X" else op)
        assert ar.cigar_string(folded) == a.cigar
    return len(cases)


def test_macro_and_layout_dependent_pairs(oracle):
    from test_gpu_align import MACRO

    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    assert check_oracle_cases(oracle, sc, [(p, r) for p, r, *_ in MACRO], T="i8", lanes=4) >= 2 * len(MACRO)
    layout = [
        (4, -2, -3, -1, b"GGACTAAGCTAACACAGGTAGGCTTTATAAAAGGTTAAAGTGCGTGAGCTAGGGTGGCTCTCACT", b"TATAAAAGGTTAAAGTGCTGTAGCTTAGGGTTGCTCTC"),
        (3, -1, -4, -1, b"TGGGGCATTTATGCGATGCAAGACAGGTCTAATATTGAAATTTATTCTAGACTATGCGAGGCCGCTCAAAGGAACCATTACCTTTTTCCGTAGGTCTCCCGATCGCGGCTAACTACTGC", b"ATAGCGATCGCAGCGCCAGGTCT"),
    ]  # SURVEY.md §7 (tests/test_gpu_align.py: test_layout_dependent_cigars)
    for ma, mi, go, ge, ref, read in layout:
        for N in (2, 64):
            check_oracle_cases(oracle, oracle.dna_scoring(ma, mi, b"N", go, ge), [(read, ref)], lanes=N)


def test_h5_against_h1_lower_case_against_upper_case(oracle, h5, h1):
    """NC_026433.1 is lower-case, NC_007362.1 upper-case: every column is X under the reference's byte equality, and the usual mix
    under ZSW_ANNOTATE_MATCH_RESIDUES; soft clips of hundreds of bases in front of the columns."""
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    assert h1[:40].islower() and h5[:40].isupper()
    cases, _ = oracle_cases(oracle, sc, [(h5, h1)])
    got = check(sc, cases)
    raw = [g for c, g in zip(cases, got) if not c["flags"] & ar.MATCH_RESIDUES]
    res = [g for c, g in zip(cases, got) if c["flags"] & ar.MATCH_RESIDUES]
    assert raw and all(s[0] == 0 and s[1] > 0 for s, _ in raw)
    assert all(s[0] > s[1] and s[0] + s[1] == r[0][1] for (s, _), r in zip(res, raw))  # an alignment that scores has more matches than not
    assert all(s[6] == raw[0][0][6] and s[7] == ar.OK for s, _ in raw + res)


@pytest.mark.parametrize("scheme", [(2, -5, -10, -1), (4, -2, -3, -1), (3, -1, -2, -2)])
def test_random_pairs(oracle, scheme):
    ma, mi, go, ge = scheme
    rng = np.random.default_rng(stable_seed("annotate", scheme))
    sc = oracle.dna_scoring(ma, mi, b"N", go, ge)
    alpha = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)
    ref = bytes(rng.choice(alpha[:4], 400))
    pairs = []
    for _ in range(110):
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
    assert check_oracle_cases(oracle, sc, pairs) >= 300


# ---- every status, hand-built ---------------------------------------------------------------------------------------------------

SEQ = b"ACGTACGTTGCAACGTAGCTAGCTAGGATCCATGCATGCAAGCTTGCA" * 4  # 192 bases
READ = SEQ[20:120]                                                # 100 of them


def status_cases():
    """(expected status, case); flags 0 unless said: ref = SEQ[20:120], query = READ"""
    M, I, D, S, N, H, P, EQ, X = (ord(c) for c in "MIDSNHP=X")
    c = lambda cigar, rr=(20, 120), **kw: case_cigar(0, READ, SEQ, 200, rr, (0, 100), cigar, **kw)
    out = [
        (ar.OK, c("100M")),
        (ar.OK, c("3=2M95=")),                                   # 3=2M whose M starts with a match: 5=...
        (ar.OK, c("5H2P40=1X59=3H")),                            # X over a matching column: counted as a match, kept as X
        (ar.OK, case_cigar(0, SEQ[20:30] + b"TTTTT" + SEQ[35:120], SEQ, 190, (20, 120), (0, 100), "10M5N5S85M")),  # N skips reference, S skips query
        (ar.REFERENCE_ENDED, c("100M1M")),                       # over-long: the reference is looked up first
        (ar.REFERENCE_ENDED, c("50M1D50M")),
        (ar.QUERY_ENDED, c("50M1I50M")),
        (ar.QUERY_ENDED, c("100M5S")),                           # found by the end checks
        (ar.QUERY_ENDED, c("101M", rr=(20, 130))),
        (ar.REFERENCE_ENDED, c("100M5N")),
        (ar.FULL_QUERY_NOT_USED, c("99M", rr=(20, 119))),        # truncated
        (ar.FULL_QUERY_NOT_USED, c("60M")),                      # ... both too short: the query is compared first
        (ar.FULL_REFERENCE_NOT_USED, c("60M40S")),
        (ar.INVALID_CIGAR_OP, c("50M1Z49M")),
        (ar.INVALID_CIGAR_OP, c("200S1Z")),                      # the end checks have not run yet
        (ar.REFERENCE_ENDED, c("101M1Z")),                       # ... but a column has
        (ar.NO_ALIGNMENT, c("100M", status=2)),
        (ar.BAD_RECORD, c("100M", rr=(120, 20))),                # ref_start > ref_end
        (ar.BAD_RECORD, c("50M0I50M")),                          # an inc of 0
        (ar.BAD_RECORD, case_of(0, READ, SEQ, rec_of(200, (20, 120), (0, 100), len(SEQ), len(READ), 2, off=0), [(100, M)])),       # n_ciglets past the end
        (ar.BAD_RECORD, case_of(0, READ, SEQ, rec_of(200, (20, 120), (0, 100), len(SEQ), len(READ), 1, off=2 ** 63), [(100, M)])),
        (ar.BAD_RECORD, case_of(0, READ, SEQ, rec_of(200, (20, 120), (0, 100), len(SEQ), len(READ), 0xFFFFFFFF, off=2 ** 64 - 2), [(100, M)])),
        (ar.BAD_RECORD, case_of(0, READ, SEQ, rec_of(200, (20, 120), (0, 100), len(SEQ) + 1, len(READ), 1), [(100, M)])),           # ref_len is not the sequence's
        (ar.BAD_RECORD, case_of(0, READ, SEQ, rec_of(200, (20, 120), (0, 100), len(SEQ), len(READ) - 1, 1), [(100, M)])),
        (ar.BAD_RECORD, case_of(0, READ, SEQ, rec_of(200, (20, 193), (0, 100), len(SEQ), len(READ), 1), [(100, M)])),               # ref_end past the sequence
        (ar.BAD_RECORD, c("4294967295H4294967295H100M")),        # equal neighbours merge beyond 32 bits
        (ar.REFERENCE_ENDED, c("4294967295M")),                  # inc = 0xffffffff
        (ar.QUERY_ENDED, c("4294967295I4294967295I100M")),
        (ar.REFERENCE_ENDED, c("4294967295D4294967295N100M")),
        (ar.QUERY_ENDED, c("100M4294967295S4294967295S")),       # the cursors do not wrap
        (ar.OK, case_of(0, READ, SEQ, rec_of(200, (20, 120), (0, 100), len(SEQ), len(READ), 1, off=3), [(7, ord("Z")), (0, M), (9, I), (100, M)])),  # other reads' ciglets are not this read's
    ]
    # a mismatch-only path: NEGATIVE_SCORE with the negative sum, counts and verbose CIGAR kept
    other = bytes(b"ACGT"[(b"ACGT".index(b) + 1) % 4] for b in READ)
    out.append((ar.NEGATIVE_SCORE, case_cigar(0, other, SEQ, 0, (20, 120), (0, 100), "100M")))
    # caller-built = / X, alternating 1M1I (70 ciglets), inverted roles
    out.append((ar.OK, case_cigar(0, READ, SEQ, 0, (20, 120), (0, 100), "1=1X" * 50)))
    ins = bytes(b for k in range(35) for b in (READ[k], ord("T")))
    out.append((ar.NEGATIVE_SCORE, case_cigar(0, ins + READ[35:], SEQ, 0, (20, 120), (0, 135), "1M1I" * 35 + "65M")))  # 100 * 2 - 35 * 10
    out.append((ar.OK, case_cigar(ar.READ_IS_REF, READ, SEQ, 200, (0, 100), (20, 120), "20S100M72S")))
    out.append((ar.FULL_REFERENCE_NOT_USED, case_cigar(ar.READ_IS_REF, READ, SEQ, 200, (0, 100), (20, 119), "20S99M73S")))
    return out


def sweep_cases():
    """M runs of 1, G, G + 1 and 2G + 3 columns with a mismatch on each side of every sweep boundary and at the first and last
    column of a run; reads of 1, G - 1, G, G + 1 bases"""
    seq = (SEQ * 3)[:420]
    out = []
    for run in (1, G, G + 1, 2 * G + 3):
        for bad in ([], [0], [run - 1], sorted({0, run - 1}), sorted({k for b in range(G, run, G) for k in (b - 1, b)}), sorted({b - 1 for b in range(G, run + 1, G)}),
                    sorted({b for b in range(G, run, G)})):
            read = bytearray(seq[7:7 + 5 + run + 4])
            for k in bad:
                read[5 + k] = ord("a")
            read[4] = ord("c")  # the columns around the run differ: they belong to other ciglets
            out.append(case_cigar(0, read, seq, 0, (12, 12 + run), (5, 5 + run), f"5S{run}M4S"))
            out.append(case_cigar(0, read, seq, 0, (10, 12 + run + 2), (3, 5 + run + 2), f"3S2X{run}M2={2}S"))
    for L in (1, G - 1, G, G + 1):
        out.append(case_cigar(0, seq[30:30 + L], seq, 0, (30, 30 + L), (0, L), f"{L}M"))
    return out


def test_every_status_and_the_merge_cases(oracle):
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    cases = status_cases()
    got = check(sc, [c for _, c in cases])
    for k, ((want, c), (stats, verbose)) in enumerate(zip(cases, got)):
        assert stats[7] == want, (k, ar.cigar_string(zip(c["inc"], c["op"])), stats)
        if want not in ar.ANNOTATED:
            assert stats[:7] == ar.ZERO and not verbose
    assert {w for w, _ in cases} == set(range(9))
    assert ar.cigar_string(got[1][1]) == "100=" and ar.cigar_string(got[2][1]) == "5H2P40=1X59=3H" and got[2][0][:2] == (100, 0)
    neg = next(g for (w, c), g in zip(cases, got) if w == ar.NEGATIVE_SCORE and len(c["inc"]) == 1)
    assert neg[0] == (0, 100, 0, 0, 0, 0, -500, ar.NEGATIVE_SCORE) and ar.cigar_string(neg[1]) == "100X"


def test_sweep_boundaries(oracle):
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    got = check(sc, sweep_cases())
    assert all(s[7] == ar.OK or s[7] == ar.NEGATIVE_SCORE for s, _ in got)


def test_malformed_records_under_sanitizers(oracle):
    """the model built with -fsanitize=address,undefined (a stand-alone executable, nothing preloaded) over the hand-built records:
    every array in a heap block of exactly its size, so an index that leaves one ends the run"""
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    check(sc, [c for _, c in status_cases()] + sweep_cases(), sanitize=True)


def test_the_symbol_is_in_every_list():
    from zoe_amd import _lib

    name = "zsw_annotate_batch"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zoe_sw.h")).read(), flags=re.S)
    assert re.search(r"\b" + name + r"\s*\(", hdr) and "zsw_alignment_stats" in hdr
    assert name in _lib.SYMBOLS and ar.STATS_DTYPE.itemsize == 32
    import ctypes

    assert ctypes.sizeof(_lib.ZswAlignmentStats) == 32 and [f[0] for f in _lib.ZswAlignmentStats._fields_] == list(ar.STATS_DTYPE.names)
    assert "zsw_*" in open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_exports.map")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "zoe_sw_gpu.rs")).read()
    assert len(re.findall(r"\b" + name + r"\(", rs)) >= 2 and "pub struct ZswAlignmentStats" in rs
    for k, v in (("OK", 0), ("REFERENCE_ENDED", 1), ("QUERY_ENDED", 2), ("FULL_QUERY_NOT_USED", 3), ("FULL_REFERENCE_NOT_USED", 4), ("INVALID_CIGAR_OP", 5),
                 ("NEGATIVE_SCORE", 6), ("NO_ALIGNMENT", 7), ("BAD_RECORD", 8)):
        assert re.search(r"ZSW_PATH_" + k + r"\s*=\s*" + str(v) + r"\b", hdr) and getattr(ar, k) == v and getattr(_lib, "PATH_" + k) == v
