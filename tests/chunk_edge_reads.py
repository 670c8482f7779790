"""A deterministic set of reads that sit on the edges of the row-chunked full pass (zsw_score.hip: seed_items,
zsw_score_v2.hpp: ScoreArgsV2::chunk_rows).

A read the seeded pass hands back against a long reference is scored in chunks of reference rows: chunk k owns rows
[kB, (k + 1)B) and walks them from row kB - V, from a zero state. Everything the launch is made of is derived HERE, from the
scoring scheme, the longest read of the batch (the read length of a fixed-length batch, the class capacity G * C of a class of a
ragged one) and the reference length, and from nothing the library exports:

  V = longest + floor(longest * maxw / gap_extend) + 2     rows a positive path can span
  B = max(4 V, 2048)                                       rows a chunk owns
  chunked  <=>  ref_len >= 8192 and 2 B <= ref_len and gap_extend > 0;  ceil(ref_len / B) chunks
  K = 8, plus 1 while K < 12 and 4^K < 32 ref_len          the k-mer length of the reference index

Every edge read must reach that pass for a known reason: it shares NO K-mer with the reference, so the seed kernel finds no
anchor and lists it. The reads are built from pieces of the reference and made K-mer-free in one of two ways,
  subs    pieces of 30 bases, one substituted base in every run of 8 (6 .. 8 < K exact bases between two), the substituted bases
          and their places redrawn until no K-mer of the read occurs in the reference (gap_open >= 10 pays for a long piece);
  exact   exact pieces of 7 .. K - 1 bases, their boundaries redrawn likewise (gap_open = 2: a substitution costs more than a gap),
with `skip` reference rows left out between two pieces, so that the designed alignment spans len + (pieces - 1) * skip rows and
its reference range is known: rows [start, end), `end` being the 1-based ref_end the library reports. Where the oracle does not
give a read's designed range, the read takes another draw (REDRAW, E_DRAW below): the construction is changed, not excused.

The edges, per (scheme, read length, reference length) and per boundary kB (k = 1 and the last chunk's):
  a  end = kB (last owned row of chunk k - 1), kB + 1 (first owned row of chunk k), end = ref_len, start = row 0
  b  the long plan ending at kB + 1, kB + 2, kB + 3: chunk k sees the path through its overlap only, chunk k - 1 sees all of it
     but its last one to three rows — an overlap of `longest` rows, or a chunk that starts a few rows late, gives a lower score
  c  the middle of the path on row kB, once inside a piece and once inside a skipped stretch
  d  a stretch of the reference copied to two further places (into chunk 1's owned rows and, where there is room, chunk 2's);
     reads from the stretch whose first occurrence ends at B - 5, B and B + 1: the same maximum in several chunks, twice in
     chunk 1 for the last two (once in its overlap, once whole in its owned rows): the first row must win. (A first occurrence
     that BEGINS above row B - V cannot be built: no positive path spans more than V rows, which is what the overlap rests on.)
  e  X + f + X: the same K-mer-free image of a window twice in one read (f: one or two bases, more in a later draw, that match
     on neither copy's diagonal), the window ending at kB + 1: equal maxima in two columns of row kB + 1, the first column must
     win. Not under gap_open = 2, where the oracle showed no tie for any draw tried
and the filler: `junk` (random reads without a K-mer of the reference) and `copies` (exact copies of the reference clear of the
duplicated stretches, which the band of the seeded pass proves; batches take every start an even number of times, so that lane
partners share an anchor). With gap_extend = 0 there is no V and no chunk: that world holds the filler only.

tests/test_chunk_edge_reads.py checks against the oracle alone that the reads sit where this says."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import strip_edge_reads as ser

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SEED = 20240
N_JUNK, N_COPY_STARTS = 96, 32

# name -> ((match, mismatch, gap_open, gap_extend), read length (0: the ragged batch of RAGGED_LENGTHS), reference length)
SCHEME_A, SCHEME_B, SCHEME_C, SCHEME_F = (2, -5, -10, -1), (2, -5, -2, -1), (6, -5, -12, -5), (3, -4, -5, 0)
WORLDS = {
    "A": (SCHEME_A, 150, 8193), "A0": (SCHEME_A, 150, 8192), "A-": (SCHEME_A, 150, 8191),
    "B": (SCHEME_B, 150, 8193), "C": (SCHEME_C, 151, 8193),
    "D": (SCHEME_A, 400, 9616), "D-": (SCHEME_A, 400, 9615), "D+": (SCHEME_A, 400, 9617),
    "E": (SCHEME_A, 0, 8193), "F": (SCHEME_F, 150, 8193),
}
RAGGED_LENGTHS = (150, 300, 600)
# e: which draw of X the world uses — (world, read length) -> draw, 0 if not listed, None: the world has no such read. With the
# first draw, under scheme C (a match 6, a one-row gap 12) the tail of the first X, read as arbitrary bases against the rows in
# front of the window, adds a few points to the second X: the oracle shows no tie, and tests/test_chunk_edge_reads.py fails; draw
# 11 is the first that ties. Under scheme B (a one-row gap costs 2) no draw tried gave a tie — a path leaves either X through a
# cheap gap and picks up chance matches — so world B has no X + X read.
E_DRAW: Dict[Tuple[str, int], Optional[int]] = {("C", 151): 11, ("B", 150): None}

# a, b, c, d: (world, read length, the read's first tag) -> draw, 0 if not listed. A designed alignment can tie with, or lose a few
# points to, a variant that swaps its last pieces for chance matches; tests/test_chunk_edge_reads.py then fails, and the read
# takes its next draw (other substituted bases, other piece boundaries — the designed rows stay)
REDRAW: Dict[Tuple[str, int, str], int] = {("B", 150, "a:end@4B"): 3, ("B", 150, "c:skip@3B"): 2}


class Params(NamedTuple):
    V: Optional[int]   # None: gap_extend = 0, no bound
    B: Optional[int]
    chunked: bool
    chunks: int        # grid rows of the chunked launch (0 if there is no B)
    K: int


def seed_k(ref_len: int) -> int:
    K = 8
    while K < 12 and 4 ** K < 32 * ref_len:
        K += 1
    return K


def chunk_params(scheme, longest: int, ref_len: int) -> Params:
    ma, _mi, _go, ge = scheme
    K = seed_k(ref_len)
    if ge == 0:
        return Params(None, None, False, 0, K)
    V = longest + (longest * ma) // -ge + 2
    B = max(4 * V, 2048)
    return Params(V, B, ref_len >= 8192 and 2 * B <= ref_len, -(-ref_len // B), K)


def class_capacity(length: int) -> int:
    """capacity G * C of the length class of a ragged batch that holds reads of `length` bases"""
    return min(g * c for g, c in ser.length_classes() if g * c >= length)


def kmer_codes(a: np.ndarray, K: int) -> np.ndarray:
    """the K-mers of every row of a 2-D array of ACGT bytes, two bits per base"""
    two = ((a >> 1) & 3).astype(np.uint32)
    n = a.shape[1] - K + 1
    code = np.zeros((a.shape[0], n), dtype=np.uint32)
    for j in range(K):
        code = (code << 2) | two[:, j:n + j]
    return code


class Plan(NamedTuple):
    kind: str            # "subs" | "exact"
    length: int          # bases of the read
    pieces: int
    skip: int            # reference rows left out between two pieces

    @property
    def span(self) -> int:
        return self.length + (self.pieces - 1) * self.skip


def plans(scheme, length: int, K: int) -> Dict[str, Plan]:
    """long: the longest span that was found to hold against the oracle for the scheme; dup: a short one, for the reads of the
    duplicated stretch; half: one gapless piece of half a read, for X + X"""
    go = -scheme[2]
    if go >= 10:
        n = max(1, length // 30)
        return {"long": Plan("subs", length, n, 20), "dup": Plan("subs", length, n, 5), "half": Plan("subs", (length - 1) // 2, 1, 0)}
    n = -(-length // 8)
    h = -(-((length - 1) // 2) // 8)
    return {"long": Plan("exact", length, n, 10), "dup": Plan("exact", length, n, 2), "half": Plan("exact", (length - 1) // 2, h, 2)}


def piece_lengths(plan: Plan) -> List[int]:
    """the planned piece lengths: 30, 30, ..., the rest in the last piece; or, exact pieces, as even as they come, the shorter
    ones in the middle (150 bases in 19 pieces: two of 7 between nine and eight of 8)"""
    if plan.kind == "subs":
        return [30] * (plan.pieces - 1) + [plan.length - 30 * (plan.pieces - 1)]
    base, rem = divmod(plan.length, plan.pieces)
    return [base + 1] * (rem - rem // 2) + [base] * (plan.pieces - rem) + [base + 1] * (rem // 2)


def plan_rows(plan: Plan, K: int, rng, ref: np.ndarray, start: int) -> np.ndarray:
    """The reference row of every base of the read whose designed alignment covers rows [start, start + plan.span).

    Exact pieces: a piece that could be one base longer at either end spells K-mers of the reference together with its neighbour
    (the row behind a piece holds the next piece's first base with probability 1/4). So the end of every piece and the start of
    the next one are moved by up to two rows each until the pieces are maximal — the row behind piece i differs from the first
    base of piece i + 1, and the row in front of piece i + 1 from the last base of piece i — with pieces of 7 .. K - 1 bases (the
    first and the last no shorter than planned: they must pay for the gap beside them), gaps of at most one row more than
    planned (gap_open 2, gap_extend 1: eleven rows cost 12, a piece of 7 earns 14), and the moves adding up to nothing, so that the read keeps its length and the alignment its first and last row."""
    lens = piece_lengths(plan)
    s_nom = start + np.cumsum([0] + [n + plan.skip for n in lens[:-1]])
    e_nom = s_nom + np.array(lens)
    if plan.kind == "subs" or plan.pieces == 1:
        return np.concatenate([np.arange(a, b) for a, b in zip(s_nom, e_nom)])
    assert 7 <= min(lens) and max(lens) < K
    for _ in range(2000):
        s, bal, pieces = start, 0, []
        for i in range(plan.pieces - 1):
            opts = []
            for d in range(-2, 3):
                for g in range(-2, 3):
                    e, s2 = int(e_nom[i]) + d, int(s_nom[i + 1]) + g
                    if (lens[0] if i == 0 else 7) <= e - s < K and 1 <= s2 - e <= plan.skip + 1 and ref[e] != ref[s2] and ref[s2 - 1] != ref[e - 1]:
                        opts.append((max(abs(bal + d - g), 2 if i < plan.pieces - 2 else 0), float(rng.random()), d, g))
            if not opts:
                break
            _, _, d, g = min(opts)
            pieces.append((s, int(e_nom[i]) + d))
            s, bal = int(s_nom[i + 1]) + g, bal + d - g
        else:
            if bal == 0 and lens[-1] <= int(e_nom[-1]) - s < K:
                pieces.append((s, int(e_nom[-1])))
                return np.concatenate([np.arange(a, b) for a, b in pieces])
    raise AssertionError(("no maximal pieces", plan, start))


class RefIndex:
    def __init__(self, ref: np.ndarray, K: int):
        self.ref, self.K = ref, K
        self.present = np.zeros(4 ** K, dtype=bool)
        self.present[kmer_codes(ref[None, :], K)[0]] = True

    def shared(self, reads: np.ndarray) -> np.ndarray:
        """per read: how many of its K-mers occur in the reference"""
        return self.present[kmer_codes(reads, self.K)].sum(axis=1)


def image(ix: RefIndex, plan: Plan, start: int, rng, tail=None) -> np.ndarray:
    """The read of `plan` whose designed alignment begins at reference row `start`, K-mer-free (with `tail(x)` the whole read made
    of the image x: X + X). Redrawn until it is."""
    ref, K = ix.ref, ix.K
    assert start >= 0 and start + plan.span <= len(ref), (start, plan, len(ref))
    for attempt in range(20000):
        rows = plan_rows(plan, K, rng, ref, start)
        assert len(rows) == plan.length and rows[0] == start and rows[-1] == start + plan.span - 1
        x = ref[rows].copy()
        if plan.kind == "subs":
            pos = np.arange(7, plan.length - 4, 8)  # never the first base, never one of the last four (what follows must pay for it)
            if plan.length - 1 - pos[-1] > K - 2:  # one more, halfway into a tail that could hold a K-mer
                pos = np.append(pos, min(plan.length - 5, pos[-1] + (plan.length - pos[-1]) // 2))
            if attempt:  # (a position whose three other bases all complete a K-mer of the reference: one base earlier)
                pos = pos - rng.integers(0, 2, len(pos))
            x[pos] = ACGT[(np.searchsorted(ACGT, x[pos]) + rng.integers(1, 4, len(pos))) % 4]
            runs = np.diff(np.concatenate([[-1], pos, [plan.length]])) - 1  # exact bases between substitutions: 6 .. 8
            assert (x[pos] != ref[rows][pos]).all() and runs.max() < K, (runs.max(), K)
        whole = x if tail is None else tail(x)
        if ix.shared(whole[None, :])[0] == 0:
            return whole
    raise AssertionError(("no K-mer-free image found", plan, start))


class Edge(NamedTuple):
    tag: str
    seq: bytes
    start: int            # designed reference range: rows [start, end), end = the 1-based ref_end
    end: int
    qrange: Tuple[int, int]  # designed query range


class ClassSet:
    """One length class of a world: its numbers, its edge reads, its filler; `pool` holds the distinct reads, edges first."""

    def __init__(self, name: str, scheme, length: int, longest: int, ix: RefIndex, rng, dup: Optional[Tuple[int, int]], avoid=()):
        self.name, self.length, self.longest = name, length, longest
        R = len(ix.ref)
        self.p = p = chunk_params(scheme, longest, R)
        self.plans = plans(scheme, length, p.K)
        self.edges: List[Edge] = []
        if p.B is not None:
            self._place(ix, R, dup)
        cand = np.zeros((0, length), dtype=np.uint8)
        while len(cand) < N_JUNK:
            c = ACGT[rng.integers(0, 4, (4000, length))]
            cand = np.concatenate([cand, c[ix.shared(c) == 0]])
        self.junk = cand[:N_JUNK]
        # copies that keep clear of every duplicated stretch: a copy that lies in one has its maximum in several rows, and the
        # band cannot prove it
        clear = np.array([s for s in range(0, R - length + 1, 3) if all(s + length <= a or b <= s for a, b in avoid)], dtype=np.int64)
        self.copy_starts = clear[np.linspace(0, len(clear) - 1, N_COPY_STARTS).astype(np.int64)]
        assert len(set(self.copy_starts.tolist())) == N_COPY_STARTS
        self.copies = np.stack([ix.ref[s:s + length] for s in self.copy_starts])
        edge_rows = [np.frombuffer(e.seq, dtype=np.uint8) for e in self.edges]
        self.pool = np.ascontiguousarray(np.concatenate(([np.stack(edge_rows)] if edge_rows else []) + [self.junk, self.copies]))
        self.n_edges, self.junk0, self.copy0 = len(self.edges), len(self.edges), len(self.edges) + N_JUNK
        assert (ix.shared(self.pool[:self.copy0]) == 0).all()

    def _place(self, ix, R, dup):
        B, n = self.p.B, self.p.chunks
        long_, dupl, half = self.plans["long"], self.plans["dup"], self.plans["half"]
        S, L = long_.span, self.length
        seen = {}

        def add(tag, plan, end):
            start = end - plan.span
            if start < 0 or end > R:
                return
            if (plan, start) in seen:  # the same read under a second name
                k = seen[(plan, start)]
                self.edges[k] = self.edges[k]._replace(tag=self.edges[k].tag + "+" + tag)
                return
            seen[(plan, start)] = len(self.edges)
            rng = np.random.default_rng([SEED, L, plan.skip, start, REDRAW.get((self.name, L, tag), 0)])  # every read its own draws
            self.edges.append(Edge(tag, image(ix, plan, start, rng).tobytes(), start, end, (0, L)))

        ks = sorted({1, n - 1}) if n >= 2 else []
        for k in ks:
            add(f"a:end@{k}B", long_, k * B)
            add(f"a:end@{k}B+1", long_, k * B + 1)
        add("a:end@ref_len", long_, R)
        add("a:start@0", long_, S)
        for k in ks:
            for j in (1, 2, 3):
                add(f"b:end@{k}B+{j}", long_, k * B + j)
        # c: the middle piece / the skipped stretch in front of it, with its middle on row kB
        lens = piece_lengths(long_)
        m = long_.pieces // 2
        piece_at = sum(lens[:m]) + m * long_.skip
        for k in sorted({1, max(1, (R - S) // B)}) if n >= 2 else []:
            add(f"c:piece@{k}B", long_, k * B - (piece_at + lens[m] // 2) + S)
            if long_.skip:
                add(f"c:skip@{k}B", long_, k * B - (piece_at - long_.skip // 2) + S)
        if dup is not None:
            for e in (B - 5, B, B + 1):
                assert dup[0] <= e - dupl.span and e <= dup[0] + dup[1]
                add(f"d:first@{'B%+d' % (e - B) if e != B else 'B'}", dupl, e)
        # e: X + f + X, the window of X ending on row kB + 1 — of the second boundary where there are three chunks, away from the
        # duplicated stretch. f: bases that match neither on the diagonal of the first X continued behind its window nor on that of
        # the second X continued in front of it, so that neither copy is extended straight through f. Draw d makes X d bases
        # shorter and f 2 d bases longer
        k = 2 if n >= 3 and 2 * B + 1 <= R else 1
        end = k * B + 1
        e_draw = E_DRAW.get((self.name, L), 0)
        if n >= 2 and end <= R and e_draw is not None:
            hl = half.length - e_draw
            half = half._replace(length=hl, pieces=1 if half.kind == "subs" else -(-hl // 8))
            s0, nf = end - half.span, L - 2 * hl
            f = np.array([[b for b in ACGT if b != ix.ref[min(end + j, R - 1)] and b != ix.ref[s0 - nf + j]][0] for j in range(nf)], dtype=np.uint8)
            seq = image(ix, half, s0, np.random.default_rng([SEED, L, e_draw]), tail=lambda x: np.concatenate([x, f, x]))
            self.edges.append(Edge(f"e:coltie@{k}B+1", seq.tobytes(), s0, end, (0, hl)))


def dup_layout(scheme, length, longest, R):
    """(source row, length, [destination rows]) of the duplicated stretch of a class, or None"""
    p = chunk_params(scheme, longest, R)
    if p.B is None:
        return None
    span = plans(scheme, length, p.K)["dup"].span
    n = max(200, span + 8)
    src = p.B + 2 - n
    dst = [d for d in (p.B + 400, 2 * p.B + 400) if d + n <= R]
    return (src, n, dst) if src >= 0 and dst else None


class World:
    def __init__(self, name: str):
        self.name = name
        self.scheme, L, R = WORLDS[name]
        self.ref_len, self.ragged = R, L == 0
        rng = np.random.default_rng([SEED, sorted(WORLDS).index(name)])
        ref = ACGT[rng.integers(0, 4, R)]
        lengths = RAGGED_LENGTHS if self.ragged else (L,)
        longest = [class_capacity(x) if self.ragged else x for x in lengths]
        dups = [dup_layout(self.scheme, x, lg, R) for x, lg in zip(lengths, longest)]
        taken = []
        for d in dups:  # all copies first: the reads are built from, and are K-mer-free against, the reference as it ends up
            if d is None:
                continue
            src, n, dst = d
            for at in [src] + dst:
                assert all(at + n <= a or b <= at for a, b in taken), (name, "the duplicated stretches overlap")
                taken.append((at, at + n))
            for at in dst:
                ref[at:at + n] = ref[src:src + n]
        self.dups = dups
        self.ref_np, self.ref = ref, ref.tobytes()
        ix = RefIndex(ref, seed_k(R))
        self.K = ix.K
        self.classes = [ClassSet(name, self.scheme, x, lg, ix, rng, None if d is None else (d[0], d[1]), taken) for x, lg, d in zip(lengths, longest, dups)]


_worlds: Dict[str, World] = {}


def world(name: str) -> World:
    """built once per process: the generator is deterministic"""
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


def batch_indices(cs: ClassSet, n_junk: int, n_copies: int, seed: int = 1) -> np.ndarray:
    """A batch as indices into cs.pool, shuffled: every edge read once, `n_junk` junk reads, `n_copies` (even) copies with every
    start an even number of times. K-mer-free reads of the batch: cs.n_edges + n_junk."""
    assert n_copies % 2 == 0
    pairs = n_copies // 2
    per = pairs // N_COPY_STARTS + (np.arange(N_COPY_STARTS) < pairs % N_COPY_STARTS)
    idx = np.concatenate([np.arange(cs.n_edges), cs.junk0 + np.arange(n_junk) % N_JUNK, np.repeat(cs.copy0 + np.arange(N_COPY_STARTS), 2 * per)])
    return idx[np.random.default_rng(seed).permutation(len(idx))]
