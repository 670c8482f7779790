"""The first band tier along its diagonals (seed_diag_kernel, zoe_amd/csrc/zsw_score_band.hip): score-only batches of reads of up to
255 bases walk the narrow band as strips of ONE column. Every result here is compared with the oracle and with the same call
under ZSW_DEBUG_SEED_STRIP_FIRST_TIER (the 16-column strips of seed_band_kernel); the debug records say which kernel walked a
read (columns per strip: 1, 16, or the second tier's 48) and, for the diverged sets, must equal the host model's values at C = 1
(tests/models/seed_band.cpp as a library; cell by cell at C = 1 without a GPU: tests/test_diag_model.py). Batches of a few
thousand reads take the two-tier path through ZSW_DEBUG_SCORE_PRUNE_ANY_SIZE."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, stable_seed

pytestmark = pytest.mark.gpu

D = 16      # the kernel's window: SEED_NARROW_WU + SEED_NARROW_WD + 1 + SEED_DIAG_SLACK diagonals, and its unrolled columns
SLACK = 1   # SEED_DIAG_SLACK
WU, WD = 8, 6
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


@pytest.fixture(scope="module")
def model():
    d = tempfile.mkdtemp(prefix="zsw_diag_model_")
    so = os.path.join(d, "libseed_band_model.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DZSW_MODEL_LIB", "-Wno-unknown-pragmas", "-o", so,
                    os.path.join(ROOT, "tests", "models", "seed_band.cpp")], check=True)
    lib = C.CDLL(so)
    lib.zsw_model_band.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 11 + [C.c_void_p]
    lib.zsw_model_band.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def ref2k():
    from zoe_amd import synth

    return synth.reference_host(2000)


def _copies(ref: bytes, rng, n: int, L: int, sub_pm: int = 20, starts=None) -> np.ndarray:
    """n reads of L bases copied from the reference (start < 0 or beyond R - L: the overhang is random), sub_pm per mille substituted"""
    r = np.frombuffer(ref, dtype=np.uint8)
    out = ACGT[rng.integers(0, 4, (n, L))]
    if starts is None:
        starts = rng.integers(0, len(r) - L + 1, n)
    for i, s in enumerate(starts):
        lo, hi = max(0, -int(s)), min(L, len(r) - int(s))
        if hi > lo:
            out[i, lo:hi] = r[int(s) + lo : int(s) + hi]
    hit = rng.integers(0, 1000, out.shape) < sub_pm
    out[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return out


def _edge_mix(ref: bytes, rng, n: int, L: int) -> np.ndarray:
    """copies from everywhere, copies whose band is clamped at row 0 (dt < wu) and at the last row (dt + len + wd > R), overhanging
    both ends, and a few unrelated reads"""
    R = len(ref)
    k = n // 8
    starts = np.concatenate([rng.integers(0, max(1, R - L + 1), n - 5 * k), rng.integers(0, WU, k), rng.integers(-min(L // 3, 12), 0, k),
                             rng.integers(max(0, R - L - WD), R - L + 1, k), rng.integers(R - L + 1, R - L + 1 + min(L // 3, 12), k)])
    reads = np.concatenate([_copies(ref, rng, len(starts), L, 20, starts), ACGT[rng.integers(0, 4, (k, L))]])
    return reads[rng.permutation(len(reads))]


def _call(za, matrix, go, ge, ref, reads, flags, records=False):
    """reads: 2-D uint8 array or a list of bytes. Returns (score, status, tier[, records]) as numpy arrays."""
    import torch

    from zoe_amd import _lib

    ctx = za.SwContext.get(0)
    if isinstance(reads, np.ndarray):
        n = reads.shape[0]
        batch = za.ReadBatch.from_fixed(torch.from_numpy(np.ascontiguousarray(reads).reshape(-1)).cuda(), reads.shape[1])
    else:
        n = len(reads)
        batch = za.ReadBatch.from_sequences(reads)
    prof = za.LocalProfilesBatch.new_with_w256(batch, matrix, go, ge)
    rec = torch.full((n, 8), -7, dtype=torch.int32, device="cuda") if records else None
    ctx.debug_set(_lib.DEBUG_SCORE_PRUNE_ANY_SIZE | flags)
    try:
        if records:
            ctx.debug_band_records(rec)
        got = prof.sw_score_from_i8(ref)
        torch.cuda.synchronize()
    finally:
        ctx.debug_band_records(None)
        ctx.debug_set(0)
    out = (got.score.cpu().numpy().view(np.uint32), got.status.cpu().numpy(), got.tier.cpu().numpy())
    return out + (rec.cpu().numpy(),) if records else out


def _oracle(za, oracle, matrix, go, ge, ref, reads):
    sc = oracle.Scoring(matrix.signed_weights(), matrix.mapping.index_map, go, ge)
    if isinstance(reads, np.ndarray):
        return oracle.batch_score_w256(8, sc, reads, ref, fixed_len=reads.shape[1], threads=8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    return oracle.batch_score_w256(8, sc, np.frombuffer(b"".join(reads), dtype=np.uint8), ref, offsets=off, threads=8)


def _both_equal_the_oracle(za, oracle, matrix, go, ge, ref, reads):
    """the default call (with its records) and the call under the strip flag against the oracle; returns the default call's records"""
    from zoe_amd import _lib

    want = _oracle(za, oracle, matrix, go, ge, ref, reads)
    s, st, t, rec = _call(za, matrix, go, ge, ref, reads, 0, records=True)
    strips = _call(za, matrix, go, ge, ref, reads, _lib.DEBUG_SEED_STRIP_FIRST_TIER)
    for name, got in (("diagonal first tier", (s, st, t)), ("16-column first tier", strips)):
        assert np.array_equal(got[1], want[1]), name
        assert np.array_equal(got[0], want[0]), name
        assert np.array_equal(got[2], want[2]), name
    return rec


def _strip_columns(rec):
    """columns per strip of the walk that last reported a read (0: no banded kernel walked it)"""
    return np.where(rec[:, 5] == -7, 0, rec[:, 7] >> 8)


@pytest.mark.parametrize("L", [D - 1, D, D + 1, 24, 25, 2 * D + 1, 150, 255, 256])
def test_read_lengths_around_the_unrolled_group_and_the_kernel_s_limit(za, oracle, ref2k, L):
    """An odd number of reads of one length: below the seeded pass's 24 bases no banded kernel runs; 24 .. 255 bases walk the
    diagonal kernel (one and a half, two groups and a column, ten groups less ten columns, sixteen less one); 256 must take the
    16-column strips. Anchors at both ends of the reference clamp the band's rows; unrelated reads are handed back."""
    rng = np.random.default_rng(stable_seed("diag-len", L))
    reads = _edge_mix(ref2k, rng, 2001, L)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    cols = _strip_columns(_both_equal_the_oracle(za, oracle, m, -10, -1, ref2k, reads))
    if L < 24:
        assert not cols.any()
    elif L <= 255:
        assert (cols == 1).mean() > 0.5 and not (cols == 16).any(), np.bincount(cols)
    else:
        assert (cols == 16).mean() > 0.5 and not (cols == 1).any(), np.bincount(cols)


def test_lane_partners_whose_anchors_are_0_1_and_2_diagonals_apart(za, oracle, ref2k):
    """Reads are paired in anchor order. Exact copies placed so that consecutive anchors differ by 0, 1 (the slack: the window's 16th
    diagonal is a band cell) and 2 (one beyond: the second read waits for the next tier), pairs 16 rows apart."""
    rng = np.random.default_rng(stable_seed("diag-pairs"))
    gaps = [0, 1, SLACK, SLACK + 1]
    starts = []
    for p in range(100):
        starts += [10 + 16 * p, 10 + 16 * p + gaps[p % 4]]
    starts.append(1700)  # an odd number of reads: the last lane holds one
    reads = _copies(ref2k, rng, len(starts), 150, 4, starts)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    rec = _both_equal_the_oracle(za, oracle, m, -10, -1, ref2k, reads)
    cols = _strip_columns(rec)
    walked = cols == 1
    spread = (rec[:, 4] - rec[:, 3])[walked]
    assert set(spread.tolist()) == {0, 1}, np.bincount(spread)
    assert (spread == 1).sum() >= 60                 # both reads of the pairs one diagonal apart
    assert (rec[walked, 6] == np.asarray(starts)[walked]).all()  # (the anchors are where the copies were taken)
    # the second reads of the pairs two apart, and only they, were left to the second tier: it pairs them with each other, 64 rows
    # apart, beyond its own slack of 32, so it walks every other one (48-column strips) and hands the rest to the full pass
    late = np.nonzero(cols != 1)[0]
    assert late.tolist() == [2 * p + 1 for p in range(100) if p % 4 == 3], late
    assert (cols[late] == 48).sum() >= len(late) // 2 and not (cols == 16).any(), cols[late]


def test_a_ragged_batch_whose_lane_partners_differ_in_length(za, oracle, ref2k):
    """Lengths 24 .. 255 side by side (padding columns in the shorter partner's half), an odd number of reads. A ragged batch runs as
    length classes, one per strip configuration, and a class is launched with its capacity as the longest read: the class of
    225 .. 256 bases (8 lanes x 32 columns) has 256 and must keep the 16-column strips, every class up to 224 (8 x 28) the diagonals."""
    rng = np.random.default_rng(stable_seed("diag-ragged"))
    reads = []
    for i in range(3001):
        L = int(rng.integers(24, 256))
        reads.append(_edge_mix(ref2k, rng, 8, L)[0].tobytes() if i % 7 else _copies(ref2k, rng, 1, L, 60)[0].tobytes())
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    cols = _strip_columns(_both_equal_the_oracle(za, oracle, m, -10, -1, ref2k, reads))
    lens = np.array([len(x) for x in reads])
    assert (cols == 1).mean() > 0.5, np.bincount(cols)
    assert not (cols[lens <= 224] == 16).any() and not (cols[lens > 224] == 1).any(), (np.bincount(cols[lens <= 224]), np.bincount(cols[lens > 224]))
    assert (cols[lens > 224] == 16).mean() > 0.5, np.bincount(cols[lens > 224])


def test_n_in_the_reads_and_a_run_of_n_in_the_reference(za, oracle, ref2k):
    rng = np.random.default_rng(stable_seed("diag-n"))
    ref = bytearray(ref2k)
    ref[900:912] = b"N" * 12
    ref[1500:1503] = b"NNN"
    ref = bytes(ref)
    reads = _edge_mix(ref, rng, 1800, 150)
    reads = np.concatenate([reads, _copies(ref, rng, 201, 150, 20, rng.integers(760, 910, 201))])  # across the run
    for i in range(0, len(reads), 3):
        at = int(rng.integers(0, 147))
        reads[i, at : at + int(rng.integers(1, 4))] = ord("N")
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    cols = _strip_columns(_both_equal_the_oracle(za, oracle, m, -10, -1, ref, reads))
    assert (cols == 1).mean() > 0.4, np.bincount(cols)


def test_unrelated_reads_only(za, oracle, ref2k):
    """No read has an anchor but by chance: the first tier leaves at its first chunk of the unanchored tail, the second tier bails out."""
    rng = np.random.default_rng(stable_seed("diag-random"))
    reads = ACGT[rng.integers(0, 4, (2001, 150))]
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    cols = _strip_columns(_both_equal_the_oracle(za, oracle, m, -10, -1, ref2k, reads))
    assert (cols != 0).mean() < 0.2


SCHEMES = [(2, -5, -10, -1), (1, -3, -5, -2), (3, -2, -5, 0), (2, -10, -10, -1)]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_scoring_schemes(za, oracle, ref2k, scheme):
    from test_gpu_bounds import diverged_reads

    ma, mi, go, ge = scheme
    rng = np.random.default_rng(stable_seed("diag-scheme", scheme))
    reads = np.concatenate([_edge_mix(ref2k, rng, 1201, 150)] + [diverged_reads(ref2k, 400, 150, r, stable_seed("diag-scheme", scheme, r)) for r in (30, 80)])
    m = za.WeightMatrix.new_dna_matrix(ma, mi, b"N")
    _both_equal_the_oracle(za, oracle, m, go, ge, ref2k, reads)


def test_kernel_values_equal_the_model_at_one_column_per_strip(za, model, ref2k):
    """The kernel's own (maximum, oa, ob) per read against the host model's with the geometry the kernel reports — C = 1 for the
    reads the first tier settles, C = 48 for those the second tier walked again — on reads with 3, 5 and 8 % substitutions
    (+ indels), 2,000 each."""
    from test_gpu_bounds import _check, diverged_reads
    from zoe_amd import _lib

    reads = np.concatenate([diverged_reads(ref2k, 2000, 150, r, stable_seed("diag-model", r)) for r in (30, 50, 80)])
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    ctx = za.SwContext.get(0)
    ctx.debug_set(_lib.DEBUG_SCORE_PRUNE_ANY_SIZE)
    try:
        walked, accepted = _check(za, model, m, -10, -1, ref2k, reads, "score", 0.9)
    finally:
        ctx.debug_set(0)
    assert accepted > 0.2 * walked
