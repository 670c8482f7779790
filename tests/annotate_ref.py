"""The test reference of zsw_annotate_batch, written from the definitions the entry point cites (plain module, imported by name
like abi_helpers): the add_state / add_ciglet merge (src/alignment/types/state.rs:130-152), to_verbose_sequence_matching
(state.rs:320-342) under both equalities, the counts, and sw_score_from_path (src/alignment/sw/mod.rs:399-454) with its errors
in that function's order. One column, one ciglet at a time; nothing here knows about lanes, sweeps or masks."""
from __future__ import annotations

import re

import numpy as np

(OK, REFERENCE_ENDED, QUERY_ENDED, FULL_QUERY_NOT_USED, FULL_REFERENCE_NOT_USED, INVALID_CIGAR_OP, NEGATIVE_SCORE, NO_ALIGNMENT,
 BAD_RECORD) = range(9)
READ_IS_REF, SHARED, MATCH_RESIDUES = 1, 2, 4
SOME = 0
ANNOTATED = (OK, FULL_QUERY_NOT_USED, FULL_REFERENCE_NOT_USED, NEGATIVE_SCORE)  # the walk stayed inside both sequences
ZERO = (0, 0, 0, 0, 0, 0, 0)  # matches, mismatches, ins_bases, del_bases, ins_runs, del_runs, path_score

STATS_DTYPE = np.dtype([("matches", "<u4"), ("mismatches", "<u4"), ("ins_bases", "<u4"), ("del_bases", "<u4"), ("ins_runs", "<u4"),
                        ("del_runs", "<u4"), ("path_score", "<i4"), ("path_status", "<u4")])


def parse_cigar(cigar: str):
    return [(int(n), ord(o)) for n, o in re.findall(r"(\d+)(.)", cigar)]


def cigar_string(ciglets) -> str:
    return "".join(f"{inc}{chr(op)}" for inc, op in ciglets)


def add_ciglet(states: list, inc: int, op: int):
    """AlignmentStates::add_ciglet"""
    if inc > 0:
        if states and states[-1][1] == op:
            states[-1] = (states[-1][0] + inc, op)
        else:
            states.append((inc, op))


def add_state(states: list, op: int):
    add_ciglet(states, 1, op)


def to_verbose(ciglets, reference: bytes, query: bytes, ref_index: int, equal) -> list:
    """AlignmentStates::to_verbose_sequence_matching; equal(query_byte, ref_byte)"""
    out, query_index = [], 0
    for inc, op in ciglets:
        if op == ord("M"):
            for k in range(inc):
                add_state(out, ord("=") if equal(query[query_index + k], reference[ref_index + k]) else ord("X"))
            query_index += inc
            ref_index += inc
        else:
            add_ciglet(out, inc, op)
            if op in b"IS=X":
                query_index += inc
            if op in b"DN=X":
                ref_index += inc
    return out


def score_from_path(ciglets, ref_in_alignment: bytes, query: bytes, weight, gap_open: int, gap_extend: int, end_checks: bool = True):
    """sw_score_from_path -> (status, score); weight(reference_byte, query_byte); gap penalties negative, as the reference holds them.
    end_checks = False: the loop alone (what the function has decided when it reaches a ciglet)"""
    score = r = q = 0
    for inc, op in ciglets:
        if op in b"M=X":
            for _ in range(inc):
                if r >= len(ref_in_alignment):
                    return REFERENCE_ENDED, 0
                if q >= len(query):
                    return QUERY_ENDED, 0
                score += weight(ref_in_alignment[r], query[q])
                q += 1
                r += 1
        elif op == ord("I"):
            score += gap_open + gap_extend * (inc - 1)
            q += inc
        elif op == ord("D"):
            score += gap_open + gap_extend * (inc - 1)
            r += inc
        elif op == ord("S"):
            q += inc
        elif op == ord("N"):
            r += inc
        elif op in b"HP":
            pass
        else:
            return INVALID_CIGAR_OP, 0
    if not end_checks:
        return OK, score
    if q < len(query):
        return FULL_QUERY_NOT_USED, 0
    if q > len(query):
        return QUERY_ENDED, 0
    if r < len(ref_in_alignment):
        return FULL_REFERENCE_NOT_USED, 0
    if r > len(ref_in_alignment):
        return REFERENCE_ENDED, 0
    if score < 0:
        return NEGATIVE_SCORE, score
    return OK, score


def counts(ciglets, reference: bytes, query: bytes, ref_index: int, equal):
    """(matches, mismatches, ins_bases, del_bases, ins_runs, del_runs) of a path that stays inside both sequences"""
    m = x = ib = db = ir = dr = 0
    q = 0
    for inc, op in ciglets:
        if op in b"M=X":
            for k in range(inc):
                if equal(query[q + k], reference[ref_index + k]):
                    m += 1
                else:
                    x += 1
        if op == ord("I"):
            ib, ir = ib + inc, ir + 1
        if op == ord("D"):
            db, dr = db + inc, dr + 1
        if op in b"M=XIS":
            q += inc
        if op in b"M=XDN":
            ref_index += inc
    return m, x, ib, db, ir, dr


def annotate_record(rec, status: int, inc, op, read: bytes, seq: bytes, flags: int, weights, index_map, gap_open: int, gap_extend: int):
    """One read of zsw_annotate_batch -> (stats tuple of 8, verbose ciglets). rec: a mapping with zsw_alignment's fields; inc / op: the
    whole ciglet arrays; seq: the context's sequence the flags name; weights[row][column] with row = non-profile residue; gap
    penalties negative."""
    if status != SOME:
        return ZERO + (NO_ALIGNMENT,), []
    reference, query = (read, seq) if flags & READ_IS_REF else (seq, read)
    off, n = int(rec["ciglet_offset"]), int(rec["n_ciglets"])
    rs, re_, qs, qe = int(rec["ref_start"]), int(rec["ref_end"]), int(rec["query_start"]), int(rec["query_end"])
    bad = (off + n > len(inc) or rs > re_ or re_ > int(rec["ref_len"]) or int(rec["ref_len"]) != len(reference)
           or qs > qe or qe > int(rec["query_len"]) or int(rec["query_len"]) != len(query))
    if bad:
        return ZERO + (BAD_RECORD,), []
    ciglets = [(int(inc[off + k]), int(op[off + k])) for k in range(n)]
    # the first of: an invalid op, an inc of 0 ("All increments must be nonzero"), a path error of the ciglets in front of it
    stop = next((k for k, (i, o) in enumerate(ciglets) if o not in b"M=XIDSNHP" or i == 0), None)
    if stop is not None:
        st, _ = score_from_path(ciglets[:stop], reference[rs:re_], query, lambda a, b: 0, 0, 0, end_checks=False)
        if st == OK:
            st = INVALID_CIGAR_OP if ciglets[stop][1] not in b"M=XIDSNHP" else BAD_RECORD
        return ZERO + (st,), []
    im = index_map

    def weight(rb, qb):
        read_b, seq_b = (rb, qb) if flags & READ_IS_REF else (qb, rb)
        return int(weights[im[read_b]][im[seq_b]]) if flags & SHARED else int(weights[im[seq_b]][im[read_b]])

    equal = (lambda a, b: im[a] == im[b]) if flags & MATCH_RESIDUES else (lambda a, b: a == b)
    st, score = score_from_path(ciglets, reference[rs:re_], query, weight, gap_open, gap_extend)
    if st not in ANNOTATED:
        return ZERO + (st,), []
    verbose = to_verbose(ciglets, reference, query, rs, equal)
    if any(i > 0xFFFFFFFF for i, _ in verbose):
        return ZERO + (BAD_RECORD,), []
    return counts(ciglets, reference, query, rs, equal) + (score, st), verbose


def annotate_batch(aln, status, inc, op, reads, seq: bytes, flags: int, weights, index_map, gap_open: int, gap_extend: int):
    """Every read -> (stats STATS_DTYPE[n], verbose records (copies of aln with n_ciglets / ciglet_offset in read order), inc, op)"""
    n = len(reads)
    stats = np.zeros(n, dtype=STATS_DTYPE)
    out = aln.copy()
    oi, oo = [], []
    for i in range(n):
        s, v = annotate_record(aln[i], int(status[i]), inc, op, reads[i], seq, flags, weights, index_map, gap_open, gap_extend)
        stats[i] = s
        out[i]["n_ciglets"], out[i]["ciglet_offset"] = len(v), len(oi)
        oi += [c[0] for c in v]
        oo += [c[1] for c in v]
    return stats, out, np.array(oi, dtype=np.uint32), np.array(oo, dtype=np.uint8)
