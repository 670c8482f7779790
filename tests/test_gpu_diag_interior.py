"""The two copies of the diagonal first tier's column loop (seed_diag_kernel, zoe_amd/csrc/zsw_seed_diag_body.inc). A wavefront of a
one-length batch whose lane partners all share their anchor and whose walks all stay inside the reference (zsw_seed_diag.hpp:
diag_walk_is_interior) takes the copy that applies no edge mask and leaves the sixteenth diagonal out; every other wavefront, and every
wavefront under ZSW_DEBUG_SEED_DIAG_MASKED, takes the masked loop. Each batch here is compared three ways: with the oracle, read for
read; all eight ints of every debug record with the same call under the flag; (maximum, oa, ob) of the first tier's records with the
host model at one column per strip (tests/models/seed_band.cpp), as tests/test_gpu_diag_groups.py does. Reads are sorted by anchor
and a wavefront takes 64 consecutive pairs of that order, so a batch of duplicated reads has coinciding pairs throughout, and which
wavefront holds which read follows from the starts. Without a GPU: tests/test_diag_interior_model.py."""
import numpy as np
import pytest

from conftest import stable_seed
from test_gpu_diag_groups import ACGT, WD, WU, _call, _copies, _equal_oracle, _first_tier, _oracle, _records_equal_the_model, model, ref2k, za  # noqa: F401

pytestmark = pytest.mark.gpu

LENGTHS = [24, 150, 255]
REFS = [300, 2000]
WAVE_READS = 128  # 64 lanes, two reads each


@pytest.fixture(scope="module")
def refs(ref2k):
    return {2000: ref2k, 300: ref2k[700:1000]}


def _interior(dtmin, dtmax, L, R):
    """diag_walk_is_interior at the narrow band"""
    return dtmin - WU >= 1 and dtmin - WU + L - 1 < R and dtmax + L + WD < R and dtmax + WD >= 0


def _interior_starts(L, R):
    return WU + 1, R - 1 - WD - L  # first and last start of an exact copy whose walk is interior


def _twice(reads):
    """every read next to its copy: equal anchors, so the pairs of the anchor order coincide whatever the anchors are"""
    return np.repeat(reads, 2, axis=0)


def _with_indel(ref: bytes, rng, L, start):
    """a copy of the reference from `start` with one insertion or deletion of one to three bases in its middle third"""
    r = np.frombuffer(ref, dtype=np.uint8)
    k, at = int(rng.integers(1, 4)), int(rng.integers(L // 3, 2 * L // 3))
    src = r[start : start + L + 3]
    if rng.integers(0, 2):
        out = np.concatenate([src[:at], src[at + k :]])
    else:
        out = np.concatenate([src[:at], ACGT[rng.integers(0, 4, k)], src[at:]])
    assert len(out) >= L
    return out[:L].copy()


def _three_ways(za, oracle, model, ref, reads, what, flags=0):
    """returns the default call's records"""
    from zoe_amd import _lib

    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    want = _oracle(oracle, m, -10, -1, ref, reads)
    new = _call(za, m, -10, -1, ref, reads, flags)
    masked = _call(za, m, -10, -1, ref, reads, flags | _lib.DEBUG_SEED_DIAG_MASKED)
    _equal_oracle(new, want, what + ": default")
    _equal_oracle(masked, want, what + ": masked loop")
    same = (new[3] == masked[3]).all(axis=1)
    assert same.all(), (what, int((~same).sum()), np.nonzero(~same)[0][:5], new[3][~same][:3], masked[3][~same][:3])
    rows = [reads[i] for i in range(len(reads))] if isinstance(reads, np.ndarray) else [np.frombuffer(x, dtype=np.uint8) for x in reads]
    _records_equal_the_model(model, m, -10, -1, ref, rows, new[3])
    return new[3]


def _walks_interior(rec, L, R):
    """per read of the first tier: would its lane's walk qualify (the record holds the lane's two anchors)"""
    first = _first_tier(rec)
    return first, np.array([bool(first[i]) and rec[i, 3] == rec[i, 4] and _interior(int(rec[i, 3]), int(rec[i, 4]), L, R) for i in range(len(rec))])


@pytest.mark.parametrize("R", REFS)
@pytest.mark.parametrize("L", LENGTHS)
def test_all_interior(za, oracle, model, refs, L, R):
    """Exact copies and copies with one 1-3-base indel, anchored mid-reference, each read twice: every wavefront qualifies."""
    ref = refs[R]
    rng = np.random.default_rng(stable_seed("diag-interior-all", L, R))
    lo, hi = _interior_starts(L, R)
    lo, hi = lo + 4, hi - 4  # (an indel moves the anchor by up to three diagonals)
    n = 1024
    starts = rng.integers(lo, hi + 1, n)
    reads = np.stack([_copies(ref, rng, L, 0, [s])[0] if i % 2 else _with_indel(ref, rng, L, int(s)) for i, s in enumerate(starts)])
    rec = _three_ways(za, oracle, model, ref, _twice(reads), f"interior L {L} R {R}")
    first, inside = _walks_interior(rec, L, R)
    assert first.mean() >= 0.5, first.mean()  # (the exact copies at least: an indel may send a read on to the second tier)
    assert inside[first].all()


@pytest.mark.parametrize("R", REFS)
@pytest.mark.parametrize("L", LENGTHS)
def test_all_edge(za, oracle, model, refs, L, R):
    """Starts 0 .. 9 and R - L - 9 .. R - L, and reads that hang over either end by 1 .. 12 bases: the masks matter in every wavefront."""
    ref = refs[R]
    rng = np.random.default_rng(stable_seed("diag-interior-edge", L, R))
    starts = list(range(0, 10)) + list(range(R - L - 9, R - L + 1)) + list(range(-12, 0)) + list(range(R - L + 1, R - L + 13))
    starts = np.array(starts * 12)
    reads = _copies(ref, rng, L, 10, starts)
    rec = _three_ways(za, oracle, model, ref, _twice(reads), f"edge L {L} R {R}")
    assert _first_tier(rec).mean() > 0.3  # (a short read that hangs over by half its length may find no anchor)


@pytest.mark.parametrize("R", REFS)
@pytest.mark.parametrize("L", LENGTHS)
def test_the_predicates_thresholds(za, oracle, model, refs, L, R):
    """One wavefront per threshold: 63 interior pairs and one pair of exact copies whose first band row is -1, 0, 1 or 2, or whose
    first row below the band in the last column is R - 2, R - 1, R or R + 1. The record holds the anchor: the construction is checked."""
    ref = refs[R]
    rng = np.random.default_rng(stable_seed("diag-interior-thresholds", L, R))
    lo, hi = _interior_starts(L, R)
    cases = [(row + WU, row >= 1) for row in (-1, 0, 1, 2)] + [(row - WD - L, row < R) for row in (R - 2, R - 1, R, R + 1)]
    for start, expect in cases:
        fill = _copies(ref, rng, L, 0, rng.integers(lo + 2, hi - 1, WAVE_READS // 2 - 1))
        reads = _twice(np.concatenate([_copies(ref, rng, L, 0, [start]), fill]))
        rec = _three_ways(za, oracle, model, ref, reads, f"threshold start {start} L {L} R {R}")
        first, inside = _walks_interior(rec, L, R)
        assert first[:2].all() and (rec[:2, 6] == start).all(), (start, rec[:2])
        assert (inside[:2] == expect).all(), (start, expect, rec[:2])
        assert inside[2:][first[2:]].all()


def test_mixed_wavefronts(za, oracle, model, refs):
    """127 interior reads and one edge read that sorts to lane 0 of the first wavefront (its lane partner, the interior read with the
    smallest anchor, is too far away to share its band and waits for the second tier); 126 interior reads and an edge read alone in
    the last lane; 64 edge + 64 interior reads, and 128 + 128: a wavefront boundary exactly between them."""
    R, L = 2000, 150
    ref = refs[R]
    rng = np.random.default_rng(stable_seed("diag-interior-mixed"))
    lo, hi = _interior_starts(L, R)
    mid = lambda c: _copies(ref, rng, L, 0, rng.integers(lo + 50, hi - 50, c))
    low_edge = lambda c: _copies(ref, rng, L, 0, rng.integers(0, WU, c))
    one_mid = _copies(ref, rng, L, 0, [lo + 10])
    batches = {
        "edge read first": np.concatenate([low_edge(1), one_mid, _twice(mid(63))]),
        "edge read last": np.concatenate([_twice(mid(63)), _copies(ref, rng, L, 0, [R - L])]),
        "64 + 64": np.concatenate([_twice(low_edge(32)), _twice(mid(32))]),
        "128 + 128": np.concatenate([_twice(low_edge(64)), _twice(mid(64))]),
    }
    for what, reads in batches.items():
        rec = _three_ways(za, oracle, model, ref, reads, what)
        first, inside = _walks_interior(rec, L, R)
        assert first.mean() > 0.9, (what, first.mean())
        assert 0 < inside.sum() < len(reads), (what, int(inside.sum()))  # (both kinds walked the tier)


def test_narrow_both_ways(za, oracle, model, refs):
    """A batch whose pairs all coincide; one with exactly one pair whose anchors differ by 1 inside an otherwise coinciding wavefront;
    an odd count (a lone last read)."""
    R, L = 2000, 150
    ref = refs[R]
    rng = np.random.default_rng(stable_seed("diag-interior-narrow"))
    lo, hi = _interior_starts(L, R)
    starts = np.sort(rng.choice(np.arange(lo + 10, hi - 10, 3), 191, replace=False))  # (three diagonals apart: no other pair within the slack)
    reads = _twice(_copies(ref, rng, L, 0, starts))
    rec = _three_ways(za, oracle, model, ref, reads[:256], "coinciding pairs")
    first, inside = _walks_interior(rec, L, R)
    assert first.all() and inside.all()
    # the pair in the middle of the first wavefront: its second read starts one row later
    apart = reads[:256].copy()
    apart[61] = _copies(ref, rng, L, 0, [starts[30] + 1])[0]
    rec = _three_ways(za, oracle, model, ref, apart, "one pair apart by 1")
    assert _first_tier(rec).all()
    wide = rec[:, 4] - rec[:, 3]
    assert wide[60] == 1 and wide[61] == 1 and (np.delete(wide, [60, 61]) == 0).all(), wide
    rec = _three_ways(za, oracle, model, ref, reads[:257], "an odd count")
    assert _first_tier(rec).all() and rec[256, 3] == rec[256, 4] == rec[256, 6]


def test_a_ragged_batch(za, oracle, model, refs):
    """The per-lane form (UNI = false) has the masked loop only: unchanged, and the flag changes nothing."""
    R = 2000
    ref = refs[R]
    rng = np.random.default_rng(stable_seed("diag-interior-ragged"))
    reads = []
    for i in range(512):
        L = LENGTHS[i % 3]
        lo, hi = _interior_starts(L, R)
        s = [0, R - L, -5][i % 7] if i % 7 < 3 else int(rng.integers(lo, hi + 1))
        row = _copies(ref, rng, L, 10, [s])[0]
        reads += [row.tobytes(), row.tobytes()]
    rec = _three_ways(za, oracle, model, ref, reads, "ragged")
    assert _first_tier(rec).mean() > 0.5
