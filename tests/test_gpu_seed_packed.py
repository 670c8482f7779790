"""The two-phase seed kernel (seed_packed_kernel, zoe_amd/csrc/zsw_score_seed.hip; zsw_seed_packed.hpp) against the kernel it
replaces for contiguous reads of one length of up to 160 bases. Every case runs twice, by default and under
ZSW_DEBUG_SEED_PLAIN_KERNEL (seed_kernel<true, .>, the body as it was), with the band records attached: scores, statuses and tiers
must equal the oracle's, and scores, statuses, tiers, zsw_prune_rescored and all eight ints of every band record — the anchor
diagonal and the (maximum, oa, ob) that rest on the seed's info word, masks and residue codes — must be the same for both kernels.
The shapes: a lone read, a full block, a block of one read behind full ones; the lengths around the tail dword, the padding of the
code rows and the staging limit (161 takes the one-pass kernel either way); base pointers that are not 16-byte aligned; reads with
runs of N, single N inside sampled k-mers, bytes outside the alphabet and unrelated reads; the reverse pass of the ranges; the
minimum-score instantiation; a second scheme and a matrix in which N has a potential. Without a GPU:
tests/test_seed_packed_model.py."""
import numpy as np
import pytest

from conftest import stable_seed

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N_READS = 4097  # sixteen full blocks and a block of one read
LENGTHS = [24, 25, 31, 32, 33, 149, 150, 151, 152, 153, 159, 160, 161]
K = 9  # seed_k_for(2000)


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


@pytest.fixture(scope="module")
def ref2k():
    from zoe_amd import synth

    return synth.reference_host(2000)


def _layout(L, spacer=2):
    """seed_layout (zsw_seed.hpp) -> the first columns of the sampled k-mers"""
    m = min(L // (K + spacer), 16)
    if L < K:
        return []
    m = max(m, 1)
    stride = L // m
    return [(stride - K) // 2 + j * stride for j in range(m)]


def _mix(ref: bytes, rng, n: int, L: int) -> np.ndarray:
    """n reads of L bases, shuffled: pieces of the reference with 1 .. 5 % substitutions; of those an eighth with a run of N, an
    eighth with one N inside a sampled k-mer, a sixteenth with bytes outside the alphabet; a tenth of all reads unrelated"""
    r = np.frombuffer(ref, dtype=np.uint8)
    starts = rng.integers(0, len(r) - L + 1, n)
    reads = r[starts[:, None] + np.arange(L)[None, :]].copy()
    pc = rng.integers(1, 6, n)
    hit = rng.integers(0, 100, reads.shape) < pc[:, None]
    reads[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    cols = _layout(L)
    for i in range(n):
        kind = i % 16
        if kind in (1, 2):
            at, run = int(rng.integers(0, L)), int(rng.integers(2, 20))
            reads[i, at : at + run] = ord("N")
        elif kind in (3, 4) and cols:
            reads[i, cols[int(rng.integers(0, len(cols)))] + int(rng.integers(0, K))] = ord("N")
        elif kind == 5:
            reads[i, rng.integers(0, L, 2)] = (ord("x"), 0xFF)
        elif kind == 6 or (kind == 7 and i % 32 == 7):
            reads[i] = ACGT[rng.integers(0, 4, L)]
    return reads[rng.permutation(n)]


def _batch(za, reads: np.ndarray, offset: int = 0):
    """The batch on the device; offset: its base pointer lies that many bytes behind an aligned one"""
    import torch

    flat = torch.from_numpy(np.ascontiguousarray(reads).reshape(-1))
    if offset:
        buf = torch.zeros(flat.numel() + offset, dtype=torch.uint8, device="cuda")
        buf[offset:] = flat.cuda()
        dev = buf[offset:]
        assert dev.data_ptr() % 16 == offset
    else:
        dev = flat.cuda()
    return za.ReadBatch.from_fixed(dev, reads.shape[1])


def _call(za, matrix, go, ge, ref, batch, n, flags, ranges=False, min_score=0):
    """-> dict of host arrays: score, status, tier (ranges: the four coordinates too), rescored, records (and counts)"""
    import torch

    from zoe_amd import _lib

    ctx = za.SwContext.get(0)
    prof = za.LocalProfilesBatch.new_with_w256(batch, matrix, go, ge)
    rec = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    ctx.debug_set(_lib.DEBUG_SCORE_PRUNE_ANY_SIZE | flags)
    out = {}
    try:
        if min_score:
            ctx.set_min_score(min_score)
        ctx.debug_band_records(rec)
        got = prof.sw_score_ranges_from_i8(za.SeqSrc.Reference(ref)) if ranges else prof.sw_score_from_i8(ref)
        torch.cuda.synchronize()
        out["rescored"] = ctx.prune_rescored()
        if min_score:
            out["counts"] = ctx.min_score_counts()
    finally:
        ctx.debug_band_records(None)
        if min_score:
            ctx.set_min_score(0)
        ctx.debug_set(0)
    out["score"] = got.score.cpu().numpy().view(np.uint32)
    out["status"] = got.status.cpu().numpy()
    out["tier"] = got.tier.cpu().numpy()
    if ranges:
        for k in ("ref_start", "ref_end", "query_start", "query_end"):
            out[k] = getattr(got, k).cpu().numpy()
    out["records"] = rec.cpu().numpy()
    return out


def _both(za, matrix, go, ge, ref, batch, n, **kw):
    """the call by the two-phase kernel and by the one-pass kernel; everything they leave must be the same"""
    from zoe_amd import _lib

    new = _call(za, matrix, go, ge, ref, batch, n, 0, **kw)
    old = _call(za, matrix, go, ge, ref, batch, n, _lib.DEBUG_SEED_PLAIN_KERNEL, **kw)
    assert sorted(new) == sorted(old)
    for k in new:
        if k == "records":
            same = (new[k] == old[k]).all(axis=1)
            assert same.all(), (int((~same).sum()), np.nonzero(~same)[0][:5], new[k][~same][:3], old[k][~same][:3])
        elif isinstance(new[k], np.ndarray):
            assert np.array_equal(new[k], old[k]), (k, np.nonzero(new[k] != old[k])[0][:8])
        else:
            assert new[k] == old[k], (k, new[k], old[k])
    return new


def _oracle(oracle, matrix, go, ge, ref, reads):
    sc = oracle.Scoring(matrix.signed_weights(), matrix.mapping.index_map, go, ge)
    return oracle.batch_score_w256(8, sc, reads, ref, fixed_len=reads.shape[1], threads=8)


def _equal_oracle(got, want, what):
    assert np.array_equal(got["status"], want[1]), what
    assert np.array_equal(got["score"], want[0]), what
    assert np.array_equal(got["tier"], want[2]), what


def _n_potential_matrix(za):
    """2 / -5 with a query N that scores 1 against every reference residue: N is not a good residue, and has the potential 1"""
    from zoe_amd.alignment import DNA_PROFILE_MAP

    w = np.full((5, 5), -5, dtype=np.int8)
    np.fill_diagonal(w, 2)
    w[4, :] = 0
    w[:, 4] = 1
    return za.WeightMatrix.new_custom(DNA_PROFILE_MAP, w)


@pytest.mark.parametrize("L", LENGTHS)
def test_every_length_around_the_tail_dword_and_the_staging_limit(za, oracle, ref2k, L):
    rng = np.random.default_rng(stable_seed("seed-packed-length", L))
    reads = _mix(ref2k, rng, N_READS, L)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    got = _both(za, m, -10, -1, ref2k, _batch(za, reads), N_READS)
    _equal_oracle(got, _oracle(oracle, m, -10, -1, ref2k, reads), L)
    walked = got["records"][:, 5] != -7
    assert walked.mean() > 0.5, walked.mean()  # (the records compare something)
    assert 0 < got["rescored"] < N_READS  # (unrelated reads: the list of reads without an anchor has members)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_edges(za, oracle, ref2k, n):
    rng = np.random.default_rng(stable_seed("seed-packed-blocks", n))
    reads = _mix(ref2k, rng, n, 150)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    got = _both(za, m, -10, -1, ref2k, _batch(za, reads), n)
    _equal_oracle(got, _oracle(oracle, m, -10, -1, ref2k, reads), n)


@pytest.mark.parametrize("offset", [1, 2, 15])
@pytest.mark.parametrize("L", [150, 157])
def test_base_pointers_that_are_not_aligned(za, oracle, ref2k, L, offset):
    rng = np.random.default_rng(stable_seed("seed-packed-offset", L, offset))
    reads = _mix(ref2k, rng, 1025, L)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    got = _both(za, m, -10, -1, ref2k, _batch(za, reads, offset), len(reads))
    _equal_oracle(got, _oracle(oracle, m, -10, -1, ref2k, reads), (L, offset))


@pytest.mark.parametrize("L", [150, 155])
def test_the_reverse_pass_of_the_ranges(za, oracle, ref2k, L):
    """sw_score_ranges on 1,024 reads: its second seeded pass reads every read back to front (SeedArgs::reversed)."""
    rng = np.random.default_rng(stable_seed("seed-packed-ranges", L))
    reads = _mix(ref2k, rng, 1024, L)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    got = _both(za, m, -10, -1, ref2k, _batch(za, reads), len(reads), ranges=True)
    _equal_oracle(got, _oracle(oracle, m, -10, -1, ref2k, reads), L)
    sc = oracle.Scoring(m.signed_weights(), m.mapping.index_map, -10, -1)
    for i in range(0, len(reads), 16):
        st, s, rr, qr, tier = oracle.cascade_score_ranges(8, 256, sc, reads[i], ref2k)
        assert st == int(got["status"][i]), i
        if st == 0:
            have = (int(got["score"][i]), (int(got["ref_start"][i]), int(got["ref_end"][i])), (int(got["query_start"][i]), int(got["query_end"][i])))
            assert have == (s, rr, qr), (i, have, (s, rr, qr))


def test_the_minimum_score_instantiation(za, oracle, ref2k):
    """ZSW_OPTION_MIN_SCORE = 225 on reads of which a tenth are unrelated: seed_packed_kernel<true> settles those by claim W's bound.
    The four counters are the same for both kernels; the reads that are not below the minimum are the oracle's."""
    from zoe_amd.alignment import SOME

    rng = np.random.default_rng(stable_seed("seed-packed-min-score"))
    reads = _mix(ref2k, rng, N_READS, 150)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    got = _both(za, m, -10, -1, ref2k, _batch(za, reads), N_READS, min_score=225)
    want = _oracle(oracle, m, -10, -1, ref2k, reads)
    below = (want[1] != SOME) | (want[0] < 225)
    assert (got["status"][below] == 4).all() and (got["score"][below] == 0).all()  # ZSW_STATUS_BELOW_MIN_SCORE
    assert np.array_equal(got["status"][~below], want[1][~below]) and np.array_equal(got["score"][~below], want[0][~below])
    assert np.array_equal(got["tier"][~below], want[2][~below])
    assert got["counts"][3] == int(below.sum()) and got["counts"][0] > 0, got["counts"]


@pytest.mark.parametrize("scheme", [(5, -4, -12, -2), "n-potential"])
def test_other_scorings(za, oracle, ref2k, scheme):
    """(5, -4, -12, -2) is one of tests/test_gpu_prune.py's schemes; its matrices ignore N, whose potential is 0 in all of them, so the
    potential of N comes from a matrix of this file's own."""
    rng = np.random.default_rng(stable_seed("seed-packed-scheme", scheme))
    reads = _mix(ref2k, rng, N_READS, 150)
    if scheme == "n-potential":
        m, go, ge = _n_potential_matrix(za), -10, -1
    else:
        m, go, ge = za.WeightMatrix.new_dna_matrix(scheme[0], scheme[1], b"N"), scheme[2], scheme[3]
    got = _both(za, m, go, ge, ref2k, _batch(za, reads), N_READS)
    _equal_oracle(got, _oracle(oracle, m, go, ge, ref2k, reads), scheme)
    assert (got["records"][:, 5] != -7).mean() > 0.5
