"""Deterministic reads that sit on the decisions of the third pass of the 3-pass alignment (zsw_threepass.hip:
threepass_kernel, zsw_capi.hip: threepass_third_pass), and a replay of three_pass.rs that says which route each read must take.

What the pass decides per read, given the bounding box [rs, re) x [qs, qe) of the two score passes (rlen = re - rs rows of the
`reference`, qlen = qe - qs residues of the sequence the profile was built from):

  shortcut   rlen == qlen and the diagonal's weights add up to the score                               route 1, classify launch
  band loop  band = |rlen - qlen| + 1, doubled while band <= (qlen - 1) / 2; an attempt is accepted when
             sw_banded_align reproduces the score and its traceback stays inside the band                route 2
  scalar     sw_scalar_align on the box                                                                  route 3

and what the host loop adds: reads that are not shortcut ("DP reads") run in a first launch whose slots hold
min(max(largest need, 64), SLOT_CAP) bytes rounded up to 64, need = rlen * qlen + rows(qlen), rows(q) = ((8 q + 15) & ~15) + 32.
In that launch a read is handed to the rerun (slots of the largest need, ciglets without limit) when
  1  rows(qlen) alone exceed the slot,
  2  a banded attempt, rows + rlen * (2 band + 1), does not fit,
  3  no attempt was accepted and the box, rows + rlen * qlen, does not fit,
  4  the alignment has more than MAXC ciglets (traceback order, the outer soft clips merged in).
The rerun starts over. `replay` and `plan` below restate exactly this over oracle/oracle.py (cascade_score_ranges for the box,
banded_align for every attempt) and the constants the library names in zsw_align.hpp (read from the source, never copied);
nothing comes from the library itself. `plan` gives, per read, the eight integers zsw_debug_threepass_records reports.

Both profile roles are replayed: "direct" (the read is the profile's sequence, the reference the other one) and "shared" (the
long sequence is the profile's, read i the `reference`), where the box's rows and columns swap.

The groups (every case is asserted from the oracle alone in tests/test_threepass_edge_reads.py):
  band      scheme (3, -4, -5, 0): one deletion / insertion of d bases in a q-base read, (q, d) in (41, 19), (42, 19): band0 = 20 =
            max_band, one attempt, accepted; (41, 20), (42, 20): band0 = 21 > max_band, scalar without an attempt
  doubling  scheme (2, -5, -10, -1): 60 matches, g inserted, 60 matches, g deleted, 60 matches — an equal-length box whose diagonal
            does not add up —, g = 1, 2, 3, 5, 9, 17: 1 .. 6 attempts, accepted bands 1, 2, 4, 8, 16, 32; and `past`: short arms
            against g, the last doubling exceeds max_band without an accepted attempt (route 3 after >= 2 attempts)
  unbanded  an attempt that reproduces the score but whose traceback leaves the band (the oracle's banded_align: UNMAPPED) was
            searched for on the CPU over two-letter reads and not found (UNBANDED below says what was tried): no such read here
  tiny      scheme (1, -1, 0, 0), free gaps: DP reads whose box has 1 .. 5 query residues (max_band 0, 0, 1, 1, 2), found by
            enumerating two-letter reads; shortcut reads with boxes of 1, 2, 3, 4, 5, 7, 8 residues (the four-bytes-per-load loop
            of diag_sum and its tail), one ending on the reference's last base, all on the read's last base
  ciglets   scheme (5, -9, -1, -1): every sixth base of a reference stretch deleted; 15 deletions and one more ciglet (a soft
            clip) are MAXC = 32 ciglets and stay, 16 deletions are 33 and go to the rerun for reason 4
  cap       scheme (3, -4, -5, 0): a setter (330 x 335 box) holds the first launch's slot at SLOT_CAP; scalar boxes that need
            exactly the slot and one row more; banded attempts nearest to the slot from both sides, first attempt and doubled
  fill      a banded attempt at band = max_band whose bytes are the (uncapped) slot exactly: see fill_group
  rows      one read long enough that rows(qlen) alone exceed SLOT_CAP, and the read one base shorter, whose rows are the slot
  reuse     the setter and more DP reads than the first launch has slots, drawn cyclically from a pool of short reads

Out of scope: a bounding box beyond 2^31 bytes and soft clips beyond 2^24 bases cannot be reached at test size."""
import os
import re
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
S_ = 0
SEED = 31337
ROLES = ("direct", "shared")

SCHEME_BAND, SCHEME_DOUBLE, SCHEME_TINY, SCHEME_CIG = (3, -4, -5, 0), (2, -5, -10, -1), (1, -1, 0, 0), (5, -9, -1, -1)


# ---- the launch's arithmetic -------------------------------------------------------------------------------------------------

def constants() -> Dict[str, int]:
    """SLOT_CAP, MAXC, BUDGET, MAX_SLOTS as zoe_amd/csrc/zsw_align.hpp names them"""
    txt = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_align.hpp")).read()
    get = lambda name: int(re.search(r"constexpr \w+ THREEPASS_%s = (\d+);" % name, txt).group(1))
    return {"SLOT_CAP": get("SLOT_CAP"), "MAXC": get("MAXC"), "BUDGET": get("SCRATCH_BUDGET"), "MAX_SLOTS": get("MAX_SLOTS")}


def rows_bytes(qlen: int) -> int:
    return ((8 * qlen + 15) & ~15) + 32


def slot_need(rlen: int, qlen: int) -> int:
    return rlen * qlen + rows_bytes(qlen)


def round64(x: int) -> int:
    return (x + 63) // 64 * 64


def slot_count(slot_bytes: int, dp_reads: int, c: Dict[str, int]) -> int:
    slots = min(max(c["BUDGET"] // slot_bytes, 64), c["MAX_SLOTS"])
    slots = min(slots, (dp_reads + 63) // 64 * 64)
    return max(64, slots // 64 * 64)


# ---- the replay of three_pass.rs ---------------------------------------------------------------------------------------------

def scoring(oracle, scheme):
    ma, mi, go, ge = scheme
    return oracle.dna_scoring(ma, mi, b"N", go, ge)


class Replay(NamedTuple):
    status: int
    score: int
    rr: Tuple[int, int]      # rows of the box: the `reference` of three_pass.rs
    qr: Tuple[int, int]      # its columns: the profile's sequence
    tier: int
    shortcut: bool
    trace: tuple             # per banded attempt of the unconstrained loop: (band, accepted, oracle status of banded_align)
    ncig: int                # ciglets of the alignment (not inverted): what the kernel's writer counts

    @property
    def rlen(self):
        return self.rr[1] - self.rr[0]

    @property
    def qlen(self):
        return self.qr[1] - self.qr[0]

    @property
    def route(self):
        return 1 if self.shortcut else 2 if self.trace and self.trace[-1][1] else 3


def replay(oracle, sc, prof: bytes, other: bytes, keep: Optional[list] = None) -> Replay:
    """three_pass.rs:21-104 for the profile of `prof` walking `other`, over the oracle's ranges and banded_align (keep: a list
    that receives the oracle's own alignment, not inverted, and its tier)"""
    st, score, rr, qr, tier = oracle.cascade_score_ranges(8, 256, sc, prof, other)
    if st != S_ or qr[0] >= qr[1]:
        if keep is not None:
            keep += [oracle.Aln(status=st if st != S_ else 2), 0]
        return Replay(st if st != S_ else 2, 0, (0, 0), (0, 0), 0, False, (), 0)
    aln, tier2, how = oracle.cascade_align_3pass(8, 256, sc, prof, other)
    if keep is not None:
        keep += [aln, tier2]
    assert aln.status == S_ and tier2 == tier and aln.score == score
    rlen, qlen = rr[1] - rr[0], qr[1] - qr[0]
    im, w = np.asarray(sc.index_map), np.asarray(sc.weights, dtype=np.int64)
    box_r, box_q = other[rr[0]:rr[1]], prof[qr[0]:qr[1]]
    if rlen == qlen:
        diag = int(w[im[np.frombuffer(box_r, dtype=np.uint8)], im[np.frombuffer(box_q, dtype=np.uint8)]].sum())
        if max(diag, 0) == score:
            assert how == 0
            return Replay(st, score, rr, qr, tier, True, (), aln.n_ciglets)
    band, max_band, trace = abs(rlen - qlen) + 1, (qlen - 1) // 2, []
    while band <= max_band:
        b = oracle.banded_align(sc, box_q, box_r, band)
        ok = b.status == S_ and b.score == score
        trace.append((band, ok, b.status))
        if ok:
            break
        band *= 2
    r = Replay(st, score, rr, qr, tier, False, tuple(trace), aln.n_ciglets)
    assert how == r.route - 1, (how, r)
    return r


def first_launch(r: Replay, slot: int, maxc: int):
    """one DP launch with `slot` bytes per read and `maxc` ciglets: (route, accepted band, attempts, why, why_band); why != 0: handed on"""
    rows = rows_bytes(r.qlen)
    if rows > slot:
        return (0, 0, 0, 1, 0)
    attempts = 0
    for band, ok, _ in r.trace:
        if rows + r.rlen * (2 * band + 1) > slot:
            return (0, 0, attempts, 2, band)
        attempts += 1
        if ok:
            return (2, band, attempts, 4 if r.ncig > maxc else 0, 0)
    if rows + r.rlen * r.qlen > slot:
        return (0, 0, attempts, 3, 0)
    return (3, 0, attempts, 4 if r.ncig > maxc else 0, 0)


def plan(replays: List[Replay], c: Dict[str, int]) -> List[Optional[Tuple[int, ...]]]:
    """the eight integers of zsw_debug_threepass_records per read of a batch (None: no alignment, the record is left alone)"""
    needs = [slot_need(r.rlen, r.qlen) for r in replays if r.status == S_ and not r.shortcut]
    slot1 = round64(min(max(max(needs, default=0), 64), c["SLOT_CAP"]))
    slot2 = round64(max(max(needs, default=0), 64))
    out = []
    for r in replays:
        if r.status != S_:
            out.append(None)
        elif r.shortcut:
            out.append((1, 0, 0, 0, 0, 0, 0, r.ncig))
        else:
            route, band, attempts, why, why_band = first_launch(r, slot1, c["MAXC"])
            if why == 0:
                out.append((route, band, attempts, 1, 0, 0, slot1, r.ncig))
            else:
                route, band, attempts, again, _ = first_launch(r, slot2, 1 << 62)
                assert again == 0
                out.append((route, band, attempts, 2, why, why_band, slot2, r.ncig))
    return out


def edge(rec) -> Tuple[int, int, int, int]:
    """(route, attempts, launch, reason): what a group is built to reach"""
    return (rec[0], rec[2], rec[3], rec[4])


# ---- the groups --------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    tag: str
    seq: bytes
    want: Optional[Tuple[int, ...]]  # direct role: (route, accepted band, attempts, launch, reason, reason's band), None: only replayed
    copies: int = 1


class Group(NamedTuple):
    name: str
    scheme: Tuple[int, int, int, int]
    ref: bytes
    cases: List[Case]
    filler: List[bytes]                      # ordinary reads the cases are spread through
    must: Dict[str, set]                     # role -> the (route, attempts, launch, reason) tuples the batch must show
    roles: Tuple[str, ...] = ROLES
    inverts: Tuple[int, ...] = (0, 1)        # the `invert` values the group's alignments are asked for


def _rng(*parts):
    return np.random.default_rng([SEED] + [int(p) for p in parts])


def _random(rng, n: int) -> bytes:
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _random3(rng, n: int) -> bytes:
    """over A, C and G: an inserted run of T matches nowhere, so no chance alignment competes with the designed one"""
    return ACGT[rng.integers(0, 3, n)].tobytes()


def _unlike(rng, like: bytes) -> bytes:
    """random bases, none equal to the base of `like` at its place"""
    a = np.frombuffer(like, dtype=np.uint8)
    return ACGT[(np.searchsorted(ACGT, a) + rng.integers(1, 4, len(a))) % 4].tobytes()


def batch_reads(g: Group, seed: int = 1) -> Tuple[List[bytes], np.ndarray]:
    """the group's batch: every case `copies` times and the filler, shuffled -> (reads, index of each read's case or -1)"""
    reads, which = [], []
    for k, cs in enumerate(g.cases):
        reads += [cs.seq] * cs.copies
        which += [k] * cs.copies
    reads += g.filler
    which += [-1] * len(g.filler)
    order = np.random.default_rng(seed).permutation(len(reads))
    return [reads[i] for i in order], np.array(which, dtype=np.int64)[order]


def band_group() -> Group:
    rng = _rng(1)
    ref = _random3(rng, 300)
    cases = []
    for q, d in ((41, 19), (42, 19), (41, 20), (42, 20)):
        fits = d + 1 <= (q - 1) // 2
        want = (2, d + 1, 1, 1, 0, 0) if fits else (3, 0, 0, 1, 0, 0)
        h, at = q // 2, 40 + q
        cases.append(Case(f"del q{q} d{d}", ref[at:at + h] + ref[at + h + d:at + q + d], want))
        at = 150 + q
        h = (q - d) // 2  # both arms pay for the gap
        cases.append(Case(f"ins q{q} d{d}", ref[at:at + h] + b"T" * d + ref[at + h:at + q - d], want))
    must = {(2, 1, 1, 0), (3, 0, 1, 0)}
    return Group("band", SCHEME_BAND, ref, cases, [], {"direct": must, "shared": must})


FILLS = ((97, 47), (93, -45))  # (q, d): band0 = max_band = (q - 1) / 2 and rlen * q + rows(q) a multiple of 64


def fill_group(q: int, d: int) -> Group:
    """A banded attempt that fills its slot to the byte WITHOUT the cap: at band = max_band = (q - 1) / 2, q odd, a band row is
    the box's row (2 band + 1 = q), the attempt needs what the box needs, and a box whose need is a multiple of 64 and the
    largest of its batch is the slot. (At the cap no banded attempt fills the slot exactly, see `nearest_banded`.)"""
    rng = _rng(8, q)
    ref = _random3(rng, 400)
    band = (q - 1) // 2
    assert q % 2 == 1 and abs(d) + 1 == band and slot_need(q + d, q) % 64 == 0
    cases = [Case(f"fills q{q} d{d}", _one_gap(None, ref, 30, q, d), (2, band, 1, 1, 0, 0), 70)]
    filler = [_one_gap(None, ref, 200 + k, 30 + k, 3 if k % 2 else -3) for k in range(12) for _ in range(10)]
    must = {(2, 1, 1, 0)}
    return Group(f"fill{q}", SCHEME_BAND, ref, cases, filler, {"direct": must}, ("direct",), (0,))


DOUBLING_G = (1, 2, 3, 5, 9, 17)
# arms a, b, c, g and the reference position of the `past` read, scheme SCHEME_CIG (a gap of g costs 1 + g, an arm earns 5 a base);
# found by trying arms of 3 .. 8 bases at three positions and keeping one the oracle aligns as designed
PAST = (3, 4, 4, 5, 100)


def _two_gaps(rng, ref: bytes, at: int, a: int, b: int, c: int, g: int) -> bytes:
    """a matches, g inserted bases (rng None: T), b matches, g reference bases left out, c matches: an equal-length box from ref[at]"""
    ins = b"T" * g if rng is None else _unlike(rng, ref[at + a:at + a + g])
    return ref[at:at + a] + ins + ref[at + a:at + a + b] + ref[at + a + b + g:at + a + b + g + c]


def doubling_group() -> Group:
    rng = _rng(2)
    ref = _random(rng, 400)
    cases = []
    for k, g in enumerate(DOUBLING_G):
        cases.append(Case(f"g{g}", _two_gaps(rng, ref, 10 + 7 * k, 60, 60, 60, g), (2, 1 << k, k + 1, 1, 0, 0)))
    must = {(2, k + 1, 1, 0) for k in range(len(DOUBLING_G))}
    return Group("doubling", SCHEME_DOUBLE, ref, cases, [], {"direct": must, "shared": must})


def past_group() -> Group:
    """the last doubling exceeds max_band: arms of a + b + c bases around g = 5 give qlen = a + g + b + c = 16, max_band = 7, and
    the attempts at 1, 2 and 4 cannot hold an excursion of g; 8 > max_band, so the scalar alignment follows"""
    ref = _random3(_rng(3), 200)
    a, b, c, g, at = PAST
    q = a + g + b + c
    attempts = len([x for x in (1, 2, 4, 8, 16) if x <= (q - 1) // 2])
    assert attempts >= 2 and g > 1 << (attempts - 1)
    cases = [Case(f"past g{g}", _two_gaps(None, ref, at, a, b, c, g), (3, 0, attempts, 1, 0, 0))]
    must = {(3, attempts, 1, 0)}
    return Group("past", SCHEME_CIG, ref, cases, [], {"direct": must, "shared": must})


def ciglet_group() -> Group:
    """The stretch starts the reference: the direct role's 32nd ciglet is the read's unrelated first base (1S); the shared role
    clips the profile's sequence, the reference, and its one clip is what follows the stretch."""
    rng = _rng(4)
    ref = _random(rng, 260)
    cases = []
    for dels, launch, why in ((15, 1, 0), (16, 2, 4)):
        src = ref[:6 * dels + 5]
        body = bytes(b for k, b in enumerate(src) if k % 6 != 5)
        lead = _unlike(rng, ref[200:201])  # no base in front of the stretch: any base is unrelated
        cases.append(Case(f"{dels} deletions", lead + body, (2, dels + 1, 1, launch, why, 0)))
    must = {(2, 1, 1, 0), (2, 1, 2, 4)}
    return Group("ciglets", SCHEME_CIG, ref, cases, [], {"direct": must, "shared": must})


# tiny: the enumeration's picks, (read, box rows x columns) per role, asserted in the CPU test
TINY_REF = b"ACCAACACCA" + b"GGGGTTTT" + b"CACAAC" + b"TG"
TINY_SHORTCUT = (b"G", b"GG", b"GGG", b"GGGG", b"GGGGT", b"GGGGTTT", b"GGGGTTTT", b"TG")


def tiny_candidates() -> List[bytes]:
    """every read of 1 .. 7 bases over A and C"""
    out = []
    for n in range(1, 8):
        for v in range(1 << n):
            out.append(bytes(b"AC"[(v >> k) & 1] for k in range(n)))
    return out


def tiny_group() -> Group:
    cases = [Case(f"shortcut {len(s)}", s, (1, 0, 0, 0, 0, 0)) for s in TINY_SHORTCUT]
    cases += [Case("enumerated", s, None) for s in tiny_candidates()]
    return Group("tiny", SCHEME_TINY, TINY_REF, cases, [], {"direct": {(1, 0, 0, 0)}, "shared": {(1, 0, 0, 0)}})


# ---- slots at the cap --------------------------------------------------------------------------------------------------------

CAP_COPIES = 200
SCALAR_FITS = ((148, 656), (166, 584), (173, 560))  # qlen x rlen with slot_need == 96 KiB exactly (asserted against SLOT_CAP)


def setter(ref: bytes, at: int) -> bytes:
    """a 330-base read with a five-base deletion: a 335 x 330 box, larger than the cap, whose first banded attempt fits"""
    return ref[at:at + 165] + ref[at + 170:at + 335]


def nearest_banded(cap: int, doublings: int):
    """(q, d, band, bytes) of the banded attempts nearest to `cap` from below (<=) and above (>): a q-base read with d bases deleted
    (d > 0) or inserted (d < 0), the attempt after `doublings` doublings; q up to 3000, |d| up to 20"""
    below = above = None
    for q in range(100, 3001):
        for d in list(range(-20, 0)) + list(range(1, 21)):
            band = (abs(d) + 1) << doublings
            rlen = q + d
            if band > (q - 1) // 2 or rlen < 50:
                continue
            v = rows_bytes(q) + rlen * (2 * band + 1)
            if v <= cap and (below is None or v > below[3]):
                below = (q, d, band, v)
            if v > cap and (above is None or v < above[3]):
                above = (q, d, band, v)
    return below, above


def _one_gap(rng, ref: bytes, at: int, q: int, d: int) -> bytes:
    """a q-base read with d reference bases deleted (d > 0) or -d bases inserted (random unlike the reference's, or T: rng None)"""
    if d > 0:
        h = q // 2
        return ref[at:at + h] + ref[at + h + d:at + q + d]
    h = (q + d) // 2  # both arms pay for the gap
    ins = b"T" * -d if rng is None else _unlike(rng, ref[at + h:at + h - d])
    return ref[at:at + h] + ins + ref[at + h:at + q + d]


def _excursion(rng, ref: bytes, at: int, q: int, d: int, g: int) -> bytes:
    """q bases, net d reference bases deleted (d > 0), with g bases inserted a third of the way and g + d deleted at two thirds:
    the path leaves the band of |d| + 1 and stays inside the doubled one when |d| + 1 < g <= 2 |d| + 2 - d"""
    a = (q - g) // 3
    b = (q - g) // 3
    c = q - g - a - b
    ins = _unlike(rng, ref[at + a:at + a + g])
    return ref[at:at + a] + ins + ref[at + a:at + a + b] + ref[at + a + b + g + d:at + a + b + g + d + c]


def short_pool(rng, ref: bytes, n: int, lo: int = 30, hi: int = 60, span: int = 300) -> List[bytes]:
    """n distinct short DP reads against ref[:span]: one indel (banded), a deletion too long for any band (scalar), two gaps"""
    out, seen = [], set()
    while len(out) < n:
        L = int(rng.integers(lo, hi + 1))
        kind = len(out) % 4
        if kind == 0:
            d = int(rng.integers(1, 6))
            s = _one_gap(rng, ref, int(rng.integers(0, span - L - d)), L, d)
        elif kind == 1:
            d = -int(rng.integers(1, 6))
            s = _one_gap(rng, ref, int(rng.integers(0, span - L)), L, d)
        elif kind == 2:
            d = int(rng.integers(L // 2, 3 * L))
            s = _one_gap(rng, ref, int(rng.integers(0, span - L - d)), L, d)
        else:
            g = int(rng.integers(1, 6))
            a = (L - g) // 3
            s = _two_gaps(rng, ref, int(rng.integers(0, span - L - g)), a, a, L - g - 2 * a, g)
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def cap_group() -> Group:
    c = constants()
    cap = c["SLOT_CAP"]
    rng = _rng(5)
    ref = _random(rng, 3200)
    cases = [Case("setter", setter(ref, 400), (2, 6, 1, 1, 0, 0))]
    for q, rl in SCALAR_FITS:
        assert slot_need(rl, q) == cap
        at = 20 + q
        cases.append(Case(f"scalar fits {q}x{rl}", _one_gap(rng, ref, at, q, rl - q), (3, 0, 0, 1, 0, 0), CAP_COPIES))
        cases.append(Case(f"scalar over {q}x{rl + 1}", _one_gap(rng, ref, at, q, rl + 1 - q), (3, 0, 0, 2, 3, 0), CAP_COPIES))
    (q, d, band, v), (q2, d2, band2, v2) = nearest_banded(cap, 0)
    cases.append(Case(f"banded fits {v}", _one_gap(rng, ref, 50, q, d), (2, band, 1, 1, 0, 0), CAP_COPIES))
    cases.append(Case(f"banded over {v2}", _one_gap(rng, ref, 60, q2, d2), (2, band2, 1, 2, 2, band2), CAP_COPIES))
    (q, d, band, v), (q2, d2, band2, v2) = nearest_banded(cap, 1)
    g, g2 = band // 2 + 1, band2 // 2 + 1
    cases.append(Case(f"doubled fits {v}", _excursion(rng, ref, 70, q, d, g), (2, band, 2, 1, 0, 0), CAP_COPIES))
    cases.append(Case(f"doubled over {v2}", _excursion(rng, ref, 80, q2, d2, g2), (2, band2, 2, 2, 2, band2), CAP_COPIES))
    filler = [s for s in short_pool(rng, ref, 400) for _ in range(6)]
    must = {(2, 1, 1, 0), (3, 0, 1, 0), (3, 0, 2, 3), (2, 1, 2, 2), (2, 2, 1, 0), (2, 2, 2, 2)}
    return Group("cap", SCHEME_BAND, ref, cases, filler, {"direct": must}, ("direct",))


def rows_group() -> Group:
    """the shortest read whose two DP rows alone exceed the cap, with three indels against a reference of its own; and the same
    read without its last base, whose rows fill the slot to the byte: it stays for the band loop, whose first attempt cannot fit"""
    cap = constants()["SLOT_CAP"]
    q = next(q for q in range(1, 1 << 20) if rows_bytes(q) > cap)
    rng = _rng(6)
    ref = _random(rng, q + 700)
    p = q // 4
    body = ref[300:300 + p] + ref[300 + p + 2:300 + 2 * p] + _unlike(rng, ref[0:3]) + ref[300 + 2 * p:300 + 3 * p] + ref[300 + 3 * p + 1:]
    read = body[:q]
    assert len(read) == q and rows_bytes(q - 1) == cap
    cases = [Case(f"rows q{q}", read, (2, 2, 2, 2, 1, 0)), Case(f"rows q{q - 1}", read[:-1], (2, 2, 2, 2, 2, 1))]
    return Group("rows", SCHEME_DOUBLE, ref, cases, [], {"direct": {(2, 2, 2, 1), (2, 2, 2, 2)}}, ("direct",), (0,))


REUSE_EXTRA, REUSE_POOL = 200, 500


def reuse_group() -> Group:
    c = constants()
    rng = _rng(7)
    ref = _random(rng, 800)
    slots = slot_count(round64(c["SLOT_CAP"]), 1 << 30, c)
    pool = short_pool(rng, ref, REUSE_POOL)
    n = slots + REUSE_EXTRA
    filler = [pool[i % len(pool)] for i in range(n)]
    must = {(2, 1, 1, 0), (3, 0, 1, 0), (2, 2, 1, 0)}
    return Group("reuse", SCHEME_BAND, ref, [Case("setter", setter(ref, 420), (2, 6, 1, 1, 0, 0))], filler, {"direct": must}, ("direct",))


# UNBANDED: the search for an attempt that reproduces the score while its traceback leaves the band (tools: none — the loop below
# is the search, run once on the CPU; tests/test_threepass_edge_reads.py asserts what it records here)
# 280,000 reads tried — 10,000 for each of four seeds under (1, -1, 0, 0), (2, -5, -10, -1), (3, -4, -5, 0), (5, -9, -1, -1),
# (1, -1, -1, 0), (2, -1, -1, -1) and (4, -2, -3, -1) — and none found: the flags of a banded matrix never point across its edge
# (the E value in front of a column's first row in the band is gap_open, below zero, and never equals a cell's score).
UNBANDED_TRIED = 280000
UNBANDED: List[Tuple[Tuple[int, int, int, int], bytes, bytes]] = []  # (scheme, reference, read)


def search_unbanded(oracle, scheme, tries: int, seed: int = 0):
    """reads over two letters against a two-letter reference: the first whose replay holds an attempt the oracle's banded_align
    answers UNMAPPED (best > 0 always: the box's first cell is a match) -> (reference, read) or None"""
    rng = np.random.default_rng([SEED, 99, seed])
    sc = scoring(oracle, scheme)
    for _ in range(tries):
        two = ACGT[rng.choice(4, 2, replace=False)]
        ref = two[rng.integers(0, 2, int(rng.integers(20, 80)))].tobytes()
        read = two[rng.integers(0, 2, int(rng.integers(8, 40)))].tobytes()
        r = replay(oracle, sc, read, ref)
        if any(st != S_ for _, _, st in r.trace):
            return ref, read
    return None


GROUPS = {"band": band_group, "doubling": doubling_group, "past": past_group, "ciglets": ciglet_group, "tiny": tiny_group,
          "cap": cap_group, "rows": rows_group, "reuse": reuse_group,
          "fill97": lambda: fill_group(*FILLS[0]), "fill93": lambda: fill_group(*FILLS[1])}
_groups: Dict[str, Group] = {}


def group(name: str) -> Group:
    """built once per process: the generator is deterministic"""
    if name not in _groups:
        _groups[name] = GROUPS[name]()
    return _groups[name]


def role_args(role: str, ref: bytes, read: bytes) -> Tuple[bytes, bytes]:
    """(profile's sequence, the other one) of a read in a role"""
    return (read, ref) if role == "direct" else (ref, read)


class Expect(NamedTuple):
    replay: Replay
    record: Optional[Tuple[int, ...]]   # plan()'s eight integers in the group's batch
    keys: Dict[int, tuple]              # invert -> oracle.Aln.key() + (tier,), or the key of a read without an alignment


_expected: Dict[Tuple[str, str], Dict[bytes, Expect]] = {}


def expected(oracle, g: Group, role: str) -> Dict[bytes, Expect]:
    """the oracle's alignment (both `invert` values) and the replayed record of every distinct read of the group's batch; once
    per process"""
    if (g.name, role) not in _expected:
        from concurrent.futures import ThreadPoolExecutor

        sc = scoring(oracle, g.scheme)
        reads = list(dict.fromkeys([cs.seq for cs in g.cases] + g.filler))

        def one(s):
            prof, other = role_args(role, g.ref, s)
            keep, keys = [], {}
            r = replay(oracle, sc, prof, other, keep)
            for inv in g.inverts:
                a, tier = keep if inv == 0 else oracle.cascade_align_3pass(8, 256, sc, prof, other, other_is_query=True)[:2]
                keys[inv] = a.key() + (tier,) if a.status == S_ else (a.status, 0, (0, 0), (0, 0), "", 0, 0)
            return r, keys

        with ThreadPoolExecutor(min(12, os.cpu_count() or 1)) as pool:
            res = list(pool.map(one, reads))
        recs = plan([r for r, _ in res], constants())
        _expected[(g.name, role)] = {s: Expect(r, rec, keys) for s, (r, keys), rec in zip(reads, res, recs)}
    return _expected[(g.name, role)]
