"""The edge reads of tests/chunk_edge_reads.py sit where the generator says — checked against the oracle alone, so that the GPU
tests built on them (tests/test_gpu_row_chunks.py) cannot pass because a read missed the chunk edge it was made for, or reached
the full pass for another reason than the one the tests count on."""
import numpy as np
import pytest

import chunk_edge_reads as cer

S_ = 0
# world -> per class (longest, V, B, chunks, chunked), K — written out, not derived: the generator's arithmetic is under test too
EXPECT = {
    "A": ([(150, 452, 2048, 5, True)], 10),
    "A0": ([(150, 452, 2048, 4, True)], 9),
    "A-": ([(150, 452, 2048, 4, False)], 9),
    "B": ([(150, 452, 2048, 5, True)], 10),
    "C": ([(151, 334, 2048, 5, True)], 10),
    "D": ([(400, 1202, 4808, 2, True)], 10),
    "D-": ([(400, 1202, 4808, 2, False)], 10),
    "D+": ([(400, 1202, 4808, 3, True)], 10),
    "E": ([(152, 458, 2048, 5, True), (304, 914, 3656, 3, True), (608, 1826, 7304, 2, False)], 10),
    "F": ([(150, None, None, 0, False)], 10),
}


@pytest.mark.parametrize("name", sorted(cer.WORLDS))
def test_chunk_numbers_and_kmer_freedom(name):
    w = cer.world(name)
    want, K = EXPECT[name]
    assert w.K == K and len(w.classes) == len(want)
    for cs, (longest, V, B, chunks, chunked) in zip(w.classes, want):
        assert (cs.longest, cs.p.V, cs.p.B, cs.p.chunks, cs.p.chunked, cs.p.K) == (longest, V, B, chunks, chunked, K), (name, cs.p)
        # no edge read and no junk read shares a K-mer with the reference (recomputed here, from the reads as the batches hold them)
        present = np.zeros(4 ** K, dtype=bool)
        present[cer.kmer_codes(w.ref_np[None, :], K)[0]] = True
        assert not present[cer.kmer_codes(cs.pool[:cs.copy0], K)].any(), name
        assert present[cer.kmer_codes(cs.pool[cs.copy0:], K)].all(), name  # the copies are copies
        assert len(cs.pool) < 400 and len({r.tobytes() for r in cs.pool}) == len(cs.pool)
        tags = "+".join(e.tag for e in cs.edges)
        if name == "F":
            assert not cs.edges  # gap_extend = 0: no bound on a path's rows, never chunked, no edges to sit on
            continue
        for must in ("a:end@1B", "a:end@1B+1", "a:end@ref_len", "a:start@0", "b:end@1B+1", "b:end@1B+2", "b:end@1B+3", "c:piece@1B", "c:skip@1B",
                     "d:first@B-5", "d:first@B", "d:first@B+1", "e:coltie@"):
            # (d needs room for a copy behind row B: every class but the 600-base one of the ragged world, which is not chunked;
            # e: the oracle shows no tie for any X + X tried under scheme B, chunk_edge_reads.E_DRAW, so world B has none)
            assert must in tags or (must[0], name, longest) in (("d", "E", 608), ("e", "B", 150)), (name, must, tags)
        # b: the long plan spans more than a read's length — an overlap of `longest` rows cannot hold it
        span = cs.plans["long"].span
        assert span > cs.longest and span < cs.p.V, (name, span)
        if name == "B":
            assert span >= 0.7 * cs.p.V, (span, cs.p.V)
        ends = {e.end for e in cs.edges}
        last = cs.p.chunks - 1
        assert {cs.p.B, cs.p.B + 1, w.ref_len} <= ends and (last * cs.p.B in ends or last * cs.p.B + 1 > w.ref_len)
        assert 0 in {e.start for e in cs.edges}
    if name in ("A", "D+"):  # the last chunk owns one row, and an alignment ends on it
        cs = w.classes[0]
        assert w.ref_len - (cs.p.chunks - 1) * cs.p.B == 1 and any(e.end == w.ref_len for e in cs.edges)
    assert cer.World(name).ref == w.ref and [c.pool.tobytes() for c in cer.World(name).classes] == [c.pool.tobytes() for c in w.classes]


@pytest.mark.parametrize("name", sorted(set(cer.WORLDS) - {"F"}))
def test_every_edge_read_sits_on_its_edge(oracle, name):
    """The oracle's ranges of every designed read are the designed ones: reference rows [start, end), the whole read as the query
    range (the first X of X + X). d: the first occurrence wins although the copies score the same — which the test shows by
    scoring the read against the reference with the first occurrence cut off. e: both halves reach the same score in the same
    row, alone and together, and the oracle reports the first one's column. World B (gap_open 2) has no e read: for none of the
    eleven X + X reads tried did the oracle show equal maxima in two columns of one row — a path leaves either copy through a gap
    that costs 2 and picks up chance matches — so the case is dropped there, not weakened (chunk_edge_reads.E_DRAW)."""
    w = cer.world(name)
    ma, mi, go, ge = w.scheme
    sc = oracle.dna_scoring(ma, mi, b"N", go, ge)
    for cs, dup in zip(w.classes, w.dups):
        res = cer.ser.oracle_map(lambda e: oracle.score_ranges("i16", 16, sc, e.seq, w.ref), cs.edges)
        junk_best = max(oracle.score("i16", 16, sc, r.tobytes(), w.ref)[1] for r in cs.junk[:16])
        for e, (st, s, rr, qr) in zip(cs.edges, res):
            print(f"{name} L {cs.length} {e.tag}: score {s} rows {rr} (designed {(e.start, e.end)}) columns {qr}; junk scores up to {junk_best}")
            assert st == S_ and rr == (e.start, e.end) and qr == e.qrange, (name, cs.length, e.tag, s, rr, (e.start, e.end), qr)
            if e.tag.startswith("d:"):
                src, n, dst = dup
                assert src <= e.start and e.end <= src + n and len(dst) >= 1
                later = w.ref[e.start + 1:]  # without the first occurrence's first row: the copies alone
                st2, s2, rr2, _ = oracle.score_ranges("i16", 16, sc, e.seq, later)
                assert (st2, s2) == (S_, s) and rr2[1] + e.start + 1 == dst[0] + (e.end - src), (e.tag, s2, rr2)
            if e.tag.startswith("e:"):
                half = e.qrange[1]
                first = oracle.score_ends("i16", 16, sc, e.seq[:half], w.ref)
                second = oracle.score_ends("i16", 16, sc, e.seq[len(e.seq) - half:], w.ref)
                both = oracle.score_ends("i16", 16, sc, e.seq, w.ref)
                assert first == second == (S_, (s, e.end, half)) and both == (S_, (s, e.end, half)), (first, second, both)
