"""A deterministic set of reads that sit on the structural edges of the strip score kernels (zsw_score_v2.hpp, zsw_score_v1.hpp).

A strip configuration (G lanes per read pair, C columns per lane) holds reads of up to W = G * C columns; a ragged batch is split
into length classes, one per configuration of ascending capacity (kBucketCfg, zsw_score.hip), so a read of the class with
capacity W and previous capacity P has a length in (P, W]. Random reads meet the places where such a kernel can be subtly wrong
by luck only; the reads below are built to sit on them, in every class:

  full, full-1, min   exact copies of the reference of W, W - 1 and P + 1 bases, placed so that their rows straddle the anchor row
                      (1,024 or 2,048: a re-base row for every period K the schemes of the tests give, and, at 2,048, the
                      boundary of the LDS staging of the reference rows) — column G*C - 1 of the last lane, live or padded
  lastlane            junk in every lane but the last, which holds C reference bases
  lastcol             junk and one base in the last column: the maximum sits in column W - 1, in every row that holds the base
  end@lane, start@lane  a 20-base copy that ends in the last column of lane G/2 - 1, or starts in the first column of lane G/2
  ins                 two 30-base halves of one reference window around six foreign bases in columns (G/2)C - 3 .. (G/2)C + 2: a
                      live F carried from lane G/2 - 1 to lane G/2
  del                 a reference window with the six rows around the anchor row left out: a live E across that row
  coltie              the same 20 bases in two lanes (equal maxima in one row)
  rowtie              a prefix of a segment that occurs twice in the reference (equal maxima in two rows: the earlier one wins)

Every class holds an odd number of reads, so the last lane pair of its launch is half empty.

and, beyond the widest configuration (reads scored tile by tile, TILE_COLS = 2,432 columns per tile): copies of 2,433, 2,470,
4,864 and 4,900 bases, and the same 20 bases in two different tiles (the fold of a tile into the read's running result).

`junk` is a letter whose row and column of the weight matrix are 0 (N under `ignoring = N`), or any letter that never matches.
tests/test_strip_edge_reads.py checks against the oracle alone that the reads do sit where this says.
"""
import os
import re
from typing import List, NamedTuple, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zoe_amd", "csrc")
REF_LEN = 4600  # longer than 2,432 + 2,048: a read of the longest class can start past row 2,048 - 2,432 and still straddle it
SEED = 12345
ANCHORS = (1024, 2048)
REPEAT = (300, 3900, 60)  # ref[300:360] is copied to ref[3900:3960]
TILE_COLS = 64 * 38


def strip_configs() -> List[Tuple[int, int]]:
    """ZSW_FOR_EACH_STRIP_CONFIG of zsw_score_v2.hpp: every (G, C) the kernels are instantiated for, in the list's order."""
    txt = open(os.path.join(CSRC, "zsw_score_v2.hpp")).read()
    body = txt.split("#define ZSW_FOR_EACH_STRIP_CONFIG(X)", 1)[1].split("constexpr", 1)[0]
    return [(int(g), int(c)) for g, c in re.findall(r"X\((\d+),\s*(\d+)\)", body)]


def length_classes() -> List[Tuple[int, int]]:
    """The length classes of a ragged batch: kCfgs[kBucketCfg[k]] of zsw_score.hip, ascending capacity."""
    txt = open(os.path.join(CSRC, "zsw_score.hip")).read()
    idx = [int(x) for x in re.search(r"kBucketCfg\[\]\s*=\s*\{([^}]*)\}", txt).group(1).split(",")]
    cfgs = strip_configs()
    return [cfgs[i] for i in idx]


class EdgeRead(NamedTuple):
    tag: str
    cls: int     # index into length_classes(); len(length_classes()) for the tiled reads
    anchor: int  # the reference row the read is built around (0: none)
    seq: bytes


def reference(alphabet: bytes = b"ACGT") -> bytes:
    rng = np.random.default_rng(SEED)
    ref = bytearray(rng.choice(np.frombuffer(alphabet, np.uint8), REF_LEN).tobytes())
    a, b, n = REPEAT
    ref[b:b + n] = ref[a:a + n]
    return bytes(ref)


def _foreign(alphabet: bytes, seg: bytes) -> bytes:
    """Bases that differ from `seg` position by position: the complement for DNA, the next letter otherwise."""
    if alphabet == b"ACGT":
        return seg.translate(bytes.maketrans(b"ACGT", b"TGCA"))
    return bytes(alphabet[(alphabet.index(b) + 1) % len(alphabet)] for b in seg)


def class_anchors(G: int, C: int) -> Tuple[int, ...]:
    """Both anchor rows, but one for the two 64-lane classes (they hold most of the bases): (64,19) around row 2,048, (64,38) around
    row 1,024, where its full-length copies cover rows 0 .. 2,431 and so straddle both."""
    if G < 64:
        return ANCHORS
    return (2048,) if C == 19 else (1024,)


def edge_reads(ref: bytes, alphabet: bytes = b"ACGT", junk: bytes = b"N") -> List[EdgeRead]:
    assert len(ref) == REF_LEN and len(junk) == 1
    J = junk

    def pad(b: bytes, L: int) -> bytes:
        assert len(b) <= L, (len(b), L)
        return b + J * (L - len(b))

    out: List[EdgeRead] = []
    classes = length_classes()
    P = 0
    for k, (G, C) in enumerate(classes):
        W, j = G * C, G // 2
        first = len(out)
        for anchor in class_anchors(G, C):
            s = max(0, anchor - W // 2)
            out.append(EdgeRead("full", k, anchor, ref[s:s + W]))
            out.append(EdgeRead("full-1", k, anchor, ref[s:s + W - 1]))
            out.append(EdgeRead("min", k, anchor, ref[s:s + P + 1]))
            out.append(EdgeRead("lastlane", k, anchor, J * (W - C) + ref[anchor - 8:anchor - 8 + C]))
            out.append(EdgeRead("end@lane", k, anchor, pad(J * (j * C - 20) + ref[anchor - 10:anchor + 10], W)))
            out.append(EdgeRead("start@lane", k, anchor, pad(J * (j * C) + ref[anchor - 10:anchor + 10], W)))
            a0, left = anchor - 40, j * C - 3 - 30
            out.append(EdgeRead("ins", k, anchor, pad(J * left + ref[a0:a0 + 30] + _foreign(alphabet, ref[anchor + 100:anchor + 106]) + ref[a0 + 30:a0 + 60], W)))
            out.append(EdgeRead("del", k, anchor, pad(ref[anchor - 32:anchor - 3] + ref[anchor + 3:anchor + 32], W)))
        out.append(EdgeRead("lastcol", k, 0, J * (W - 1) + ref[7:8]))
        out.append(EdgeRead("coltie", k, 0, pad(ref[500:520] + J * C + ref[500:520], W)))
        n = min(REPEAT[2], W)
        out.append(EdgeRead("rowtie", k, 0, pad(ref[REPEAT[0]:REPEAT[0] + n], P + 1 if P + 1 >= n else W)))
        assert (len(out) - first) % 2 == 1 and all(P < len(r.seq) <= W for r in out[first:]), (G, C)
        P = W
    tiled = len(classes)
    ref2 = ref + ref
    for L in (TILE_COLS + 1, 2470, 2 * TILE_COLS, 4900):
        out.append(EdgeRead("tiled", tiled, 0, ref2[200:200 + L]))
    # the same 20 bases in tiles 0 and 1, and in tiles 1 and 2: equal score in the same row, the earlier tile's column is the answer.
    # Junk scores 0, so a path rides its diagonal at no cost: three foreign bases behind the first copy take 3 mismatches off what
    # arrives at the second copy that way
    seg, stop = ref[500:520], _foreign(alphabet, ref[520:523])
    out.append(EdgeRead("tiletie", tiled, 0, pad(J * 100 + seg + stop + J * (TILE_COLS - 23) + seg, 2600)))
    out.append(EdgeRead("tiletie", tiled, 0, pad(J * (TILE_COLS + 100) + seg + stop + J * (TILE_COLS - 23) + seg, 5000)))
    # the maximum ends in the last column of tile 0 / starts in the first column of tile 1
    out.append(EdgeRead("end@tile", tiled, 0, pad(J * (TILE_COLS - 20) + ref[1014:1034], 2500)))
    out.append(EdgeRead("start@tile", tiled, 0, pad(J * TILE_COLS + ref[1014:1034], 2500)))
    return out


def concat(reads: List[bytes]):
    """(bases uint8[total], offsets uint64[n + 1]) of a ragged batch."""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), off


def oracle_map(fn, reads: List[bytes], threads: int = 16):
    """[fn(read) for read in reads] on a thread pool: the oracle's calls release the interpreter lock."""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max(1, min(threads, os.cpu_count() or 1))) as pool:
        return list(pool.map(fn, reads))
