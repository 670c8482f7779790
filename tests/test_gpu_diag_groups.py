"""The k-mer events of the diagonal first tier, group of sixteen columns by group (seed_diag_kernel, zoe_amd/csrc/zsw_score_band.hip;
zsw_seed_diag.hpp: seed_group_patterns). A batch of reads of one length derives a group's column patterns once per wavefront, on
scalar registers; a ragged batch, or any batch under ZSW_DEBUG_SEED_DIAG_LANE_EVENTS, once per lane and read. Both forms must give
the oracle's results, the host model's values at one column per strip (tests/models/seed_band.cpp as a library) and, read for read,
each other's debug records. The table row that enters the window is addressed by a byte offset that wraps above row 0 and is
clamped to the neutral entry behind the last row: a reference far shorter than its reads keeps every walk outside it on one side
or the other. Without a GPU: tests/test_diag_events_model.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, stable_seed

pytestmark = pytest.mark.gpu

WU, WD = 8, 6  # SEED_NARROW_WU, SEED_NARROW_WD
SEED_DN, SEED_DM, SEED_TOL = 4, 4, 8  # zsw_score_seed.hpp
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
# the shortest read the seed accepts, both sides of the group edges at 32 and 48, the workload's length and its neighbour, the longest
# read the kernel takes
LENGTHS = [24, 31, 32, 33, 47, 48, 49, 150, 151, 255]
N_READS = 4097  # 4,096 and one: the last lane has no partner


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


@pytest.fixture(scope="module")
def model():
    d = tempfile.mkdtemp(prefix="zsw_diag_groups_model_")
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


def _copies(ref: bytes, rng, L: int, sub_pm: int, starts) -> np.ndarray:
    """reads of L bases copied from the reference at `starts` (the part that hangs over either end is random), sub_pm per mille substituted"""
    r = np.frombuffer(ref, dtype=np.uint8)
    out = ACGT[rng.integers(0, 4, (len(starts), L))]
    for i, s in enumerate(starts):
        lo, hi = max(0, -int(s)), min(L, len(r) - int(s))
        if hi > lo:
            out[i, lo:hi] = r[int(s) + lo : int(s) + hi]
    hit = rng.integers(0, 1000, out.shape) < sub_pm
    out[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return out


def _mix(ref: bytes, rng, n: int, L: int) -> np.ndarray:
    """n reads of L bases: copies with 2 % and 5 % substitutions; copies with one to three N (the sampled k-mers cover two thirds of
    the columns or more: most N fall inside one, and its bit leaves the masks); copies whose band is clamped at row 0 (anchor < wu)
    and at the last row; copies that hang over either end; unrelated reads"""
    R = len(ref)
    k = n // 20
    over = max(1, min(L // 3, 12))
    anywhere = lambda c: rng.integers(0, max(1, R - L + 1), c)
    holes = _copies(ref, rng, L, 20, anywhere(3 * k))
    for row in holes:
        row[rng.integers(0, L, int(rng.integers(1, 4)))] = ord("N")
    parts = [_copies(ref, rng, L, 50, anywhere(5 * k)), holes,
             _copies(ref, rng, L, 20, rng.integers(0, min(WU, R - L + 1), k)), _copies(ref, rng, L, 20, rng.integers(max(0, R - L - WD), R - L + 1, k)),
             _copies(ref, rng, L, 20, rng.integers(-over, 0, k)), _copies(ref, rng, L, 20, rng.integers(R - L + 1, R - L + 1 + over, k)),
             ACGT[rng.integers(0, 4, (k // 2, L))]]
    rest = n - sum(len(p) for p in parts)
    reads = np.concatenate(parts + [_copies(ref, rng, L, 20, anywhere(rest))])
    return reads[rng.permutation(len(reads))]


def _call(za, matrix, go, ge, ref, reads, flags):
    """reads: 2-D uint8 array or a list of bytes. Returns (score, status, tier, records)."""
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
    rec = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    ctx.debug_set(_lib.DEBUG_SCORE_PRUNE_ANY_SIZE | flags)
    try:
        ctx.debug_band_records(rec)
        got = prof.sw_score_from_i8(ref)
        torch.cuda.synchronize()
    finally:
        ctx.debug_band_records(None)
        ctx.debug_set(0)
    return got.score.cpu().numpy().view(np.uint32), got.status.cpu().numpy(), got.tier.cpu().numpy(), rec.cpu().numpy()


def _oracle(oracle, matrix, go, ge, ref, reads):
    sc = oracle.Scoring(matrix.signed_weights(), matrix.mapping.index_map, go, ge)
    if isinstance(reads, np.ndarray):
        return oracle.batch_score_w256(8, sc, reads, ref, fixed_len=reads.shape[1], threads=8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    return oracle.batch_score_w256(8, sc, np.frombuffer(b"".join(reads), dtype=np.uint8), ref, offsets=off, threads=8)


def _first_tier(rec):
    """the reads whose last report came from the diagonal kernel (one column per strip)"""
    return (rec[:, 5] != -7) & ((rec[:, 7] >> 8) == 1)


def _records_equal_the_model(model, matrix, go, ge, ref: bytes, rows, rec):
    """(maximum, oa, ob) of every read the first tier reports against the host model with the geometry of the record, at C = 1"""
    w = np.ascontiguousarray(matrix.signed_weights().astype(np.int32))
    idx = matrix.mapping.index_map
    ref_idx = np.ascontiguousarray(idx[np.frombuffer(ref, dtype=np.uint8)])
    K = 8
    while K < 12 and (1 << (2 * K)) < 32 * len(ref):
        K += 1
    out = np.zeros(8, dtype=np.int32)
    bad = []
    for i in np.nonzero(_first_tier(rec))[0]:
        q = np.ascontiguousarray(idx[rows[i]])
        g = rec[i]
        n_strips, wu, wd = int(g[5] & 0xff), int((g[5] >> 8) & 0xfff), int((g[5] >> 20) & 0xfff)
        assert n_strips >= len(q) and (wu, wd) == (WU, WD), (i, n_strips, wu, wd)  # (the columns of the longer lane partner)
        rc = model.zsw_model_band(w.ctypes.data, w.shape[0], -go, -ge, ref_idx.ctypes.data, len(ref_idx), q.ctypes.data, len(q), K, SEED_DN, SEED_DM, SEED_TOL, 1,
                                  n_strips, wu, wd, int(g[3]), int(g[4]), -1, out.ctypes.data)
        assert rc == 0 and out[0] == 1, f"read {i}: the model finds no anchor where the kernel walked a band"
        assert out[1] == g[6], f"read {i}: anchor diagonal {g[6]} (kernel) vs {out[1]} (model)"
        got = (int(g[0]), max(int(g[1]), 0), max(int(g[2]), 0))
        want = (int(out[2]), max(int(out[3]), 0), max(int(out[4]), 0))
        if got != want:
            bad.append((int(i), got, want, (n_strips, int(g[3]), int(g[4]))))
    assert not bad, f"{len(bad)} reads differ, first: {bad[:5]} (maximum2, oa, ob) kernel vs model"


def _equal_oracle(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[2], want[2]), what


@pytest.mark.parametrize("L", LENGTHS)
def test_one_length_uniform_and_per_lane_events(za, oracle, model, ref2k, L):
    """4,097 reads of one length: the default call (patterns once per wavefront) and the call under the flag (once per lane) equal
    the oracle and each other, records included; the first tier's records equal the model."""
    from zoe_amd import _lib

    rng = np.random.default_rng(stable_seed("diag-groups", L))
    reads = _mix(ref2k, rng, N_READS, L)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    want = _oracle(oracle, m, -10, -1, ref2k, reads)
    uni = _call(za, m, -10, -1, ref2k, reads, 0)
    lane = _call(za, m, -10, -1, ref2k, reads, _lib.DEBUG_SEED_DIAG_LANE_EVENTS)
    _equal_oracle(uni, want, "patterns per wavefront")
    _equal_oracle(lane, want, "patterns per lane")
    first = _first_tier(uni[3])
    assert first.mean() > 0.5, first.mean()
    same = (uni[3] == lane[3]).all(axis=1)
    assert same.all(), (int((~same).sum()), uni[3][~same][:3], lane[3][~same][:3])
    _records_equal_the_model(model, m, -10, -1, ref2k, [reads[i] for i in range(len(reads))], uni[3])


def test_a_ragged_batch_of_those_lengths(za, oracle, model, ref2k):
    """The same lengths side by side in one launch (lane partners with different layouts, so different patterns in the two halves)."""
    rng = np.random.default_rng(stable_seed("diag-groups-ragged"))
    per = {L: _mix(ref2k, rng, N_READS // len(LENGTHS) + 1, L) for L in LENGTHS}
    reads = []
    for i in range(N_READS):
        L = LENGTHS[int(rng.integers(0, len(LENGTHS)))]
        reads.append(per[L][i % len(per[L])].tobytes())
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    got = _call(za, m, -10, -1, ref2k, reads, 0)
    _equal_oracle(got, _oracle(oracle, m, -10, -1, ref2k, reads), "ragged")
    assert _first_tier(got[3]).mean() > 0.5
    _records_equal_the_model(model, m, -10, -1, ref2k, [np.frombuffer(x, dtype=np.uint8) for x in reads], got[3])


def test_reads_of_255_bases_around_a_reference_of_40_rows(za, oracle, model):
    """Every row of a walk's window lies above row 0 or behind the last row for most of its columns: the entering row's byte offset
    wraps above the reference and is clamped behind it. Reads that hold the whole reference at every offset, with a few substitutions."""
    from zoe_amd import _lib, synth

    ref = synth.reference_host(2000)[700:740]
    rng = np.random.default_rng(stable_seed("diag-groups-short-ref"))
    reads = ACGT[rng.integers(0, 4, (N_READS, 255))]
    r = np.frombuffer(ref, dtype=np.uint8)
    for i in range(N_READS):
        at = int(rng.integers(0, 255 - len(r) + 1))
        reads[i, at : at + len(r)] = r
        if i % 3 == 0:
            reads[i, at + int(rng.integers(0, len(r)))] = ACGT[rng.integers(0, 4)]
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    want = _oracle(oracle, m, -10, -1, ref, reads)
    uni = _call(za, m, -10, -1, ref, reads, 0)
    lane = _call(za, m, -10, -1, ref, reads, _lib.DEBUG_SEED_DIAG_LANE_EVENTS)
    _equal_oracle(uni, want, "patterns per wavefront")
    _equal_oracle(lane, want, "patterns per lane")
    assert np.array_equal(uni[3], lane[3])
    assert _first_tier(uni[3]).mean() > 0.5  # (an exact copy of the reference anchors a read, and its band holds the whole copy)
    _records_equal_the_model(model, m, -10, -1, ref, [reads[i] for i in range(len(reads))], uni[3])
