"""The edge reads of tests/strip_edge_reads.py sit where the generator says — checked against the oracle alone, so that the GPU
tests built on them (tests/test_gpu_strip_edges.py) cannot pass because a read missed the edge it was made for."""
import pytest

import strip_edge_reads as ser

S_ = 0
# (match, mismatch, gap_open, gap_extend): the re-base period of score_kernel_v2 is 2,048 / 1,024 / 64 rows / none
SCHEMES = [(2, -5, -10, -1), (6, -5, -12, -5), (5, -4, -120, -100), (3, -4, -5, 0)]


def test_the_class_table_follows_the_sources():
    cfgs, classes = ser.strip_configs(), ser.length_classes()
    assert len(cfgs) == 21 and len(classes) == 19
    caps = [g * c for g, c in classes]
    assert caps == sorted(set(caps)) and caps[-1] == ser.TILE_COLS
    assert set(cfgs) - set(classes) == {(8, 19), (32, 5)}  # reached by fixed-length batches only
    assert ser.REF_LEN > ser.TILE_COLS + 2048


def test_the_generator_is_deterministic_and_fills_every_class():
    ref = ser.reference()
    reads = ser.edge_reads(ref)
    assert reads == ser.edge_reads(ser.reference()) and len(reads) < 1024
    assert ref[300:360] == ref[3900:3960]
    classes = ser.length_classes()
    for k, (G, C) in enumerate(classes):
        mine = [r for r in reads if r.cls == k]
        P = classes[k - 1][0] * classes[k - 1][1] if k else 0
        assert len(mine) % 2 == 1 and all(P < len(r.seq) <= G * C for r in mine)
        assert {r.tag for r in mine} == {"full", "full-1", "min", "lastlane", "end@lane", "start@lane", "ins", "del", "lastcol", "coltie", "rowtie"}
        assert {len(r.seq) for r in mine} >= {G * C, G * C - 1, P + 1}
    tiled = sorted(len(r.seq) for r in reads if r.cls == len(classes))
    assert tiled[0] == ser.TILE_COLS + 1 and 2 * ser.TILE_COLS in tiled and tiled[-1] > 2 * ser.TILE_COLS
    # the 25-letter variant: same geometry, other letters
    alpha = b"ACDEFGHIKLMNPQRSTVWY"
    prot = ser.edge_reads(ser.reference(alpha), alpha, b"X")
    assert [(r.tag, r.cls, len(r.seq)) for r in prot] == [(r.tag, r.cls, len(r.seq)) for r in reads]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_every_read_sits_on_its_edge(oracle, scheme):
    ma, mi, go, ge = scheme
    sc = oracle.dna_scoring(ma, mi, b"N", go, ge)
    ref = ser.reference()
    reads = ser.edge_reads(ref)
    classes = ser.length_classes()
    res = ser.oracle_map(lambda r: oracle.score_ranges("i16", 16, sc, r.seq, ref), reads)
    # gaps of six cost go + 5 ge: with a 30-base half worth 30 * match, the alignment bridges them unless ge = 100
    gaps_bridge = go + 5 * ge > -30 * ma
    assert gaps_bridge == (ge != -100)
    seen = {}
    for r, (st, s, rr, qr) in zip(reads, res):
        assert st == S_, (r.tag, r.cls)
        assert s > 0 and rr[0] < rr[1] <= len(ref) and qr[0] < qr[1] <= len(r.seq)
        if r.cls == len(classes):
            if r.tag == "tiled":
                assert qr[1] - qr[0] == min(len(r.seq), ser.REF_LEN - 200) and s == ma * (qr[1] - qr[0])
            elif r.tag == "tiletie":
                # the earlier tile's copy; with free gap extension a path leaves the first copy through one long gap and picks up
                # chance matches, so the two copies do not tie there (the read is an ordinary one under that scheme)
                assert ge == 0 or (s == 20 * ma and qr[1] % ser.TILE_COLS == 120 and qr[1] < len(r.seq) - ser.TILE_COLS)
            elif r.tag == "end@tile":
                assert qr[1] == ser.TILE_COLS
            else:
                assert r.tag == "start@tile" and qr[0] == ser.TILE_COLS
            continue
        G, C = classes[r.cls]
        W = G * C
        seen.setdefault((r.cls, r.tag), []).append(r.anchor)
        if r.tag in ("full", "lastlane", "lastcol"):
            assert qr[1] == len(r.seq) == W, (r.tag, G, C)
        if r.tag in ("full", "full-1"):
            assert qr == (0, len(r.seq)) and s == ma * len(r.seq) and rr[0] < r.anchor < rr[1], (r.tag, G, C)
            if G == 64 and C == 38:
                assert rr[0] < 1024 and 2048 < rr[1]
        if r.tag == "min" and len(r.seq) > W // 2 + 1:  # long enough to reach the anchor row from where the copies start
            assert rr[0] < r.anchor < rr[1], (G, C)
        if r.tag == "lastlane":
            assert qr[0] >= W - C
        if r.tag == "lastcol":
            assert qr == (W - 1, W) and s == ma
        if r.tag == "end@lane":
            assert qr[1] % C == 0 and qr[1] == (G // 2) * C, (G, C)
        if r.tag == "start@lane":
            assert qr[0] % C == 0 and qr[0] == (G // 2) * C, (G, C)
        if r.tag in ("ins", "del"):
            if gaps_bridge:
                assert (rr[1] - rr[0]) != (qr[1] - qr[0]), (r.tag, G, C)
                if r.tag == "ins":
                    assert qr[0] < (G // 2) * C - 3 and qr[1] > (G // 2) * C + 3
                else:
                    assert rr[0] < r.anchor - 3 and rr[1] > r.anchor + 3
            # (gap_extend = 100: the two halves stay apart — nothing to assert, the read is an ordinary one there)
        if r.tag == "rowtie":
            assert rr[1] == ser.REPEAT[0] + min(ser.REPEAT[2], W) and rr[1] < ser.REPEAT[1], (G, C)
        # coltie: which of the two columns answers is the oracle's business (the kernels must report the same one)
    for k, (G, C) in enumerate(classes):
        for tag in ("full", "full-1", "min", "lastlane", "end@lane", "start@lane", "ins", "del"):
            assert tuple(seen[(k, tag)]) == ser.class_anchors(G, C), (G, C, tag)
