"""The test reference of zsw_pileup_batch and zsw_consensus_from_counts, written from the definitions the entry points cite (plain
module, imported by name like annotate_ref): pairwise_align_with (src/alignment/pairwise.rs:26-65) column by column, the bins of
NucleotideCounts (src/composition/by_position/mod.rs) and plurality_acgtn. A dict of counters; nothing here knows about lanes,
difference arrays or prefix sums."""
from __future__ import annotations

from collections import Counter

import numpy as np

READ_IS_REF, SHARED, CLEAR = 1, 2, 8
KEEP_UNCOVERED = 1
SOME = 0
A, C, G, T, N, GAP, OTHER, INVALID = range(8)  # zsw_site_counts: the bins of one site


def bin_of(b: int) -> int:
    """the bin of a byte: A C G T/U N in either case, `-`, the other IUPAC letters in either case and `.`, everything else"""
    ch = chr(b)
    if ch in "Aa":
        return A
    if ch in "Cc":
        return C
    if ch in "Gg":
        return G
    if ch in "TtUu":
        return T
    if ch in "Nn":
        return N
    if ch == "-":
        return GAP
    if ch in "RYSWKMBDHVryswkmbdhv.":
        return OTHER
    return INVALID


def aligned_columns(reference: bytes, query: bytes, ciglets, ref_index: int, ref_end: int):
    """pairwise_align_with as a list of columns (ref position | None, ref_aln byte, query position | None, query_aln byte), or None
    where the function would panic or leave [ref_index, ref_end) of the reference or the query: an op outside MIDNSHP=X, a slice
    past a sequence. An inc of 0 is no alignment either ("All increments must be nonzero")."""
    cols, q = [], 0
    r = ref_index
    for inc, op in ciglets:
        if inc == 0 or op not in b"MIDNSHP=X":
            return None
        if op in b"M=XDN" and r + inc > ref_end:
            return None
        if op in b"M=XIS" and q + inc > len(query):
            return None
        for k in range(inc if op in b"M=XDNI" else 0):
            if op in b"M=X":
                cols.append((r + k, reference[r + k], q + k, query[q + k]))
            elif op == ord("D"):
                cols.append((r + k, reference[r + k], None, ord("-")))
            elif op == ord("N"):
                cols.append((r + k, reference[r + k], None, ord("N")))
            elif op == ord("I"):
                cols.append((None, ord("-"), q + k, query[q + k]))
        if op in b"M=XDN":
            r += inc
        if op in b"M=XIS":
            q += inc
    return cols


def record_columns(rec, inc, op, read: bytes, seq: bytes, flags: int):
    """the columns of one record, or None for a record that does not count"""
    reference, query = (read, seq) if flags & READ_IS_REF else (seq, read)
    off, n = int(rec["ciglet_offset"]), int(rec["n_ciglets"])
    rs, re_, qs, qe = int(rec["ref_start"]), int(rec["ref_end"]), int(rec["query_start"]), int(rec["query_end"])
    if (off + n > len(inc) or rs > re_ or re_ > int(rec["ref_len"]) or int(rec["ref_len"]) != len(reference)
            or qs > qe or qe > int(rec["query_len"]) or int(rec["query_len"]) != len(query)):
        return None
    ciglets = [(int(inc[off + k]), int(op[off + k])) for k in range(n)]
    return aligned_columns(reference, query, ciglets, rs, re_)


def pileup(aln, status, inc, op, reads, seq: bytes, flags: int, counts=None, ins=None):
    """Every read -> (counts (len, 8) uint32, ins (len + 1, 2) uint32, n_bad); counts / ins: the tables to add to.
    reads: a list of bytes; seq: the context's sequence the flags name"""
    L = len(seq)
    sites, runs, bases = Counter(), Counter(), Counter()
    n_bad = 0
    for i in range(len(reads)):
        if int(status[i]) != SOME:
            continue
        cols = record_columns(aln[i], inc, op, reads[i], seq, flags)
        if cols is None:
            n_bad += 1
            continue
        add_record(sites, runs, bases, cols, flags, aln[i], inc, op)
    out = np.zeros((L, 8), dtype=np.uint64) if counts is None or flags & CLEAR else np.asarray(counts, dtype=np.uint64).copy()
    out_ins = np.zeros((L + 1, 2), dtype=np.uint64) if ins is None or flags & CLEAR else np.asarray(ins, dtype=np.uint64).copy()
    for (pos, b), v in sites.items():
        out[pos, b] += v
    for p, v in runs.items():
        out_ins[p, 0] += v
    for p, v in bases.items():
        out_ins[p, 1] += v
    return (out & 0xFFFFFFFF).astype(np.uint32), (out_ins & 0xFFFFFFFF).astype(np.uint32), n_bad


def add_record(sites, runs, bases, cols, flags, rec, inc, op):
    """What one record adds. Without READ_IS_REF the sequence is the reference row and the read the query row: every column with a
    reference position counts the bin of the query row's byte (`-` under D, `N` under N) there, and an I ciglet is an insertion in
    front of the reference cursor. With READ_IS_REF the rows change places: the sequence's positions are the query's, they count
    the bin of the reference row's byte (`-` under I), a D ciglet is the insertion, and the N bytes of the query row are no positions
    of the sequence, so they count nothing. One run per ciglet, as the CIGAR spells them: 2I3I are two runs."""
    swap = bool(flags & READ_IS_REF)
    off, n = int(rec["ciglet_offset"]), int(rec["n_ciglets"])
    r, q, c = int(rec["ref_start"]), 0, 0
    for k in range(n):
        i, o = int(inc[off + k]), int(op[off + k])
        seq_cursor = q if swap else r
        if o in b"M=XDNI":
            mine = cols[c:c + i]
            c += i
            for rp, rb, qp, qb in mine:
                pos, byte = (qp, rb) if swap else (rp, qb)
                if pos is not None:
                    sites[(pos, bin_of(byte))] += 1
            if (o == ord("D") if swap else o == ord("I")):
                runs[seq_cursor] += 1
                bases[seq_cursor] += i
        if o in b"M=XDN":
            r += i
        if o in b"M=XIS":
            q += i


def composition(s: bytes):
    """to_base_counts of a string: one site"""
    out = [0] * 8
    for b in s:
        out[bin_of(b)] += 1
    return out


def plurality_acgtn(bins) -> int:
    """NucleotideCounts::plurality_acgtn: the largest of A C G T N, the earlier one on a tie"""
    best, at = int(bins[0]), 0
    for i in range(1, 5):
        if int(bins[i]) > best:
            best, at = int(bins[i]), i
    return b"ACGTN"[at]


def consensus(counts, flags: int = 0, fallback: bytes | None = None) -> bytes:
    out = bytearray()
    for pos, bins in enumerate(counts):
        if flags & KEEP_UNCOVERED and not any(int(x) for x in bins[:5]):
            out.append(fallback[pos])
        else:
            out.append(plurality_acgtn(bins))
    return bytes(out)
