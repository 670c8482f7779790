"""Reads from either strand (include/zoe_sw.h: zsw_score_strands_batch_from, zsw_orient_batch, zsw_align_3pass_strands_batch_from).

The contract: with rc(read) = the read reversed and complemented, F = f(read) and R = f(rc(read)) for an existing entry point f,
the strand-aware result is F unless R ranks strictly higher (OVERFLOWED > SOME by score > UNMAPPED = EMPTY); out_strand says which,
and everything else is bit for bit what f returns for that orientation. The expected values come from the oracle run on the
reads and on reverse complements made here in Python, selected by that rule; "≡ existing" checks compare with the existing GPU
call on both copies instead. The kernel's own values (supports, whole-reference bounds, first strand) are pinned to the host
model (tests/models/strand_bound.cpp built as a library), which the CPU suite checks against the full Gotoh matrix."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import abi_helpers as ah
from abi_helpers import S_, O_, U_, E_
from conftest import ROOT, stable_seed

pytestmark = pytest.mark.gpu

SEED_TOL, SEED_MIN_LEN = 8, 24  # zsw_score_seed.hpp
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _complement_table() -> bytes:
    """IUPAC nucleotide complement, case preserved, every other byte itself (written here, not taken from the library)"""
    t = bytearray(range(256))
    pairs = {"A": "T", "T": "A", "C": "G", "G": "C", "U": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B",
             "D": "H", "H": "D", "N": "N"}
    for a, b in pairs.items():
        t[ord(a)] = ord(b)
        t[ord(a.lower())] = ord(b.lower())
    return bytes(t)


COMP = _complement_table()


def rc(read: bytes, table: bytes = COMP) -> bytes:
    return bytes(read)[::-1].translate(table)


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


@pytest.fixture(scope="module")
def model():
    d = tempfile.mkdtemp(prefix="zsw_strand_model_")
    so = os.path.join(d, "libstrand_model.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DZSW_MODEL_LIB", "-Wno-unknown-pragmas", "-o", so,
                    os.path.join(ROOT, "tests", "models", "strand_bound.cpp")], check=True)
    lib = C.CDLL(so)
    lib.zsw_model_strand_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p]
    lib.zsw_model_strand_reads.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.zsw_model_strand_settled.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_int]
    return lib


@pytest.fixture(autouse=True)
def _defaults(za):
    """every test starts and ends with the context's defaults"""
    from zoe_amd import _lib

    ctx = za.SwContext.get(0)
    yield
    ctx.debug_set(0)
    ctx.set_option(_lib.OPTION_EXACT_PRUNING, 1)
    ctx.set_complement(None)
    ctx.debug_strand_records(None)


# ---- reads and expected values -----------------------------------------------------------------------------------------------

def mutated(rng, r: np.ndarray, n: int, L: int, rate: float) -> list:
    """copies of pieces of the reference with `rate` substitutions and, for a tenth of that per base, single-base indels"""
    out = []
    for _ in range(n):
        pos = int(rng.integers(0, len(r) - L - 8))
        q = r[pos:pos + L + 8].copy()
        hit = np.nonzero(rng.random(len(q)) < rate)[0]
        q[hit] = ACGT[(np.searchsorted(ACGT, q[hit]) + rng.integers(1, 4, len(hit))) % 4]
        for _k in range(int(rng.binomial(L, rate / 10))):
            p = int(rng.integers(10, L - 10))
            q = np.insert(q, p, ACGT[rng.integers(0, 4)]) if rng.integers(0, 2) else np.delete(q, p)
        out.append(q[:L].tobytes())
    return out


def mixed_strand_reads(ref: bytes, n: int, L: int, seed: int, rates=(0.01, 0.05, 0.12), random_share=0.02) -> list:
    """n reads of L bases: equal parts at the given divergence rates plus some random reads, every other read from the reverse strand"""
    rng = np.random.default_rng(seed)
    r = np.frombuffer(ref, dtype=np.uint8)
    n_random = int(round(n * random_share))
    per = (n - n_random) // len(rates)
    reads = []
    for k, rate in enumerate(rates):
        reads += mutated(rng, r, per if k + 1 < len(rates) else n - n_random - per * (len(rates) - 1), L, rate)
    reads += [ACGT[rng.integers(0, 4, L)].tobytes() for _ in range(n_random)]
    order = rng.permutation(n)
    reads = [reads[i] for i in order]
    return [rc(q) if i % 2 else q for i, q in enumerate(reads)]


def oracle_scores(o, sc, reads: list, ref: bytes, width: int = 8):
    """score, status, tier of sw_score_from_i{width} (w256) for every read through the batch oracle; an empty read is EMPTY"""
    n = len(reads)
    full = np.array([len(q) > 0 for q in reads])
    score, status, tier = np.zeros(n, dtype=np.uint32), np.full(n, E_, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    keep = [q for q in reads if q]
    if keep:
        off = np.zeros(len(keep) + 1, dtype=np.uint64)
        np.cumsum([len(q) for q in keep], out=off[1:])
        cat = np.frombuffer(b"".join(keep), dtype=np.uint8)
        score[full], status[full], tier[full] = o.batch_score_w256(width, sc, cat, ref, offsets=off, threads=ah.ORACLE_THREADS)
    return score, status, tier


def rank(score, status):
    score, status = np.asarray(score, dtype=np.uint64), np.asarray(status)
    return np.where(status == O_, np.uint64(2) << np.uint64(32), np.where(status == S_, (np.uint64(1) << np.uint64(32)) | score, np.uint64(0)))


def by_contract(F, R):
    """(score, status, tier, strand) of the contract from the two orientations' (score, status, tier)"""
    rev = rank(R[0], R[1]) > rank(F[0], F[1])
    return tuple(np.where(rev, r, f) for f, r in zip(F, R)) + (rev.astype(np.uint8),)


def expected(o, sc, reads: list, ref: bytes, table: bytes = COMP):
    return by_contract(oracle_scores(o, sc, reads, ref), oracle_scores(o, sc, [rc(q, table) for q in reads], ref))


def batch_of(za, reads: list):
    import torch

    lens = {len(q) for q in reads}
    if len(lens) == 1 and 0 not in lens:
        flat = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
        return za.ReadBatch.from_fixed(torch.from_numpy(flat).cuda(), len(reads[0]))
    return za.ReadBatch.from_sequences(reads)


def gpu_strands(za, matrix, go, ge, reads: list, ref: bytes, width: int = 8):
    prof = za.LocalProfilesBatch.new_with_w256(batch_of(za, reads), matrix, go, ge)
    got = getattr(prof, f"sw_score_strands_from_i{width}")(ref)
    import torch

    torch.cuda.synchronize()
    return (got.score.cpu().numpy().view(np.uint32), got.status.cpu().numpy(), got.tier.cpu().numpy(), got.strand.cpu().numpy())


def assert_result(got, want, what: str):
    """score, status and strand of every read; the tier wherever there is a score (as the other -m gpu tests compare it)"""
    for k, name in ((1, "status"), (0, "score"), (3, "strand")):
        bad = np.nonzero(got[k] != want[k])[0]
        assert not len(bad), f"{what}: `{name}` differs at {len(bad)} reads, first {list(bad[:5])}: got {got[k][bad[:5]]}, want {want[k][bad[:5]]}"
    some = want[1] == S_
    assert np.array_equal(got[2][some], want[2][some]), f"{what}: tiers differ"


@pytest.fixture(scope="module")
def mixed(za, oracle):
    """the mixed-strand set of the first two tests and its expected values, computed once"""
    from zoe_amd import synth

    ref = synth.reference_host(2000)
    reads = mixed_strand_reads(ref, 4096, 150, stable_seed("strands-mixed"))
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    F, R = oracle_scores(oracle, sc, reads, ref), oracle_scores(oracle, sc, [rc(q) for q in reads], ref)
    return {"ref": ref, "reads": reads, "F": F, "R": R, "want": by_contract(F, R)}


# ---- mixed strands -------------------------------------------------------------------------------------------------------------

def test_mixed_strands_equal_the_oracle_with_and_without_the_proof(za, mixed):
    """4,096 reads of 150 bases, half of them from the reverse strand, at 1 / 5 / 12 % divergence plus 2 % random reads"""
    from zoe_amd import _lib

    ctx = za.SwContext.get(0)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    want = mixed["want"]
    assert 0.4 < want[3].mean() < 0.6
    got = gpu_strands(za, m, -10, -1, mixed["reads"], mixed["ref"])
    assert_result(got, want, "exact pruning on")
    counts = ctx.strand_counts()
    assert counts[0] > 0 and counts[1] > 0, counts
    assert counts[0] + counts[1] + counts[2] == 4096 and counts[3] == int(want[3].sum()), counts
    # bit for bit what the existing call returns for the chosen orientation (≡ existing), the tier of every read included
    fwd = za.LocalProfilesBatch.new_with_w256(batch_of(za, mixed["reads"]), m, -10, -1).sw_score_from_i8(mixed["ref"])
    rev = za.LocalProfilesBatch.new_with_w256(batch_of(za, [rc(q) for q in mixed["reads"]]), m, -10, -1).sw_score_from_i8(mixed["ref"])
    for k, name in enumerate(("score", "status", "tier")):
        f, r = getattr(fwd, name).cpu().numpy(), getattr(rev, name).cpu().numpy()
        assert np.array_equal(got[k].view(f.dtype), np.where(got[3] == 1, r, f)), name
    ctx.set_option(_lib.OPTION_EXACT_PRUNING, 0)
    off = gpu_strands(za, m, -10, -1, mixed["reads"], mixed["ref"])
    assert_result(off, want, "exact pruning off")
    assert all(np.array_equal(a, b) for a, b in zip(got, off))
    assert ctx.strand_counts() == (0, 0, 4096, int(want[3].sum()))


# ---- the kernel pinned to the model --------------------------------------------------------------------------------------------

def _k_for(ref_len: int) -> int:
    K = 8
    while K < 12 and (1 << (2 * K)) < 32 * ref_len:
        K += 1
    return K


def _check_records(za, model, matrix, go, ge, reads: list, ref: bytes, F, R):
    """every value of zsw_debug_strand_records against the model, and the settled counters against the model's rule applied to
    the oracle's scores; returns the counters"""
    import torch

    ctx = za.SwContext.get(0)
    n = len(reads)
    rec = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    ctx.debug_strand_records(rec)
    try:
        gpu_strands(za, matrix, go, ge, reads, ref)
    finally:
        ctx.debug_strand_records(None)
    rec = rec.cpu().numpy()
    counts = ctx.strand_counts()
    w = np.ascontiguousarray(matrix.signed_weights().astype(np.int32))
    idx = np.asarray(matrix.mapping.index_map, dtype=np.uint8)
    comp_idx = np.arange(32, dtype=np.uint8)
    for b in b"ACGTN":
        comp_idx[idx[b]] = idx[COMP[b]]
    ref_idx = np.ascontiguousarray(idx[np.frombuffer(ref, dtype=np.uint8)])
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(q) for q in reads], out=off[1:])
    q_idx = np.ascontiguousarray(idx[np.frombuffer(b"".join(reads) or b"\0", dtype=np.uint8)])
    out = np.zeros((n, 5), dtype=np.int32)
    assert model.zsw_model_strand_batch(w.ctypes.data, w.shape[0], -go, -ge, ref_idx.ctypes.data, len(ref_idx), q_idx.ctypes.data, off.ctypes.data, n,
                                        _k_for(len(ref)), SEED_TOL, SEED_MIN_LEN, comp_idx.ctypes.data, out.ctypes.data) == 0
    bad = np.nonzero((rec[:, :5] != out).any(axis=1))[0]
    assert not len(bad), f"{len(bad)} reads differ, first: {[(int(i), rec[i, :5].tolist(), out[i].tolist()) for i in bad[:5]]} (kernel, model)"
    first = out[:, 4]
    sp = np.where(first == 1, R[0], F[0])
    some = np.where(first == 1, R[1], F[1]) == S_
    uo = np.where(first == 1, out[:, 2], out[:, 3])
    settled = np.array([model.zsw_model_strand_settled(int(some[i]), int(sp[i]), int(uo[i]), int(first[i])) for i in range(n)], dtype=bool)
    assert np.array_equal(rec[:, 5] == 1, settled)
    assert counts[:3] == (int((settled & (first == 0)).sum()), int((settled & (first == 1)).sum()), int((~settled).sum())), counts
    return counts


def test_kernel_values_equal_the_model_on_the_mixed_reads(za, model, mixed):
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    counts = _check_records(za, model, m, -10, -1, mixed["reads"], mixed["ref"], mixed["F"], mixed["R"])
    assert counts[0] > 1000 and counts[1] > 1000  # (not vacuous: most of the 1 % and 5 % reads are settled by proof)


def test_kernel_values_equal_the_model_on_ragged_and_adversarial_reads(za, model, oracle):
    """2,000 reads of the model's own generator (copies, chimeras of both strands, reads over the ends, long gaps, reads of 1 to
    30 bases, random reads, N) of 8 to 260 bases against a reference with an inverted repeat, a palindrome and N runs"""
    from zoe_amd import synth

    refa = bytearray(synth.reference_host(2000))
    refa[900:960] = rc(bytes(refa[300:360]))            # an inverted repeat
    refa[1400:1430] = rc(bytes(refa[1370:1400]))        # a palindrome
    for at, k in ((500, 1), (650, 3), (1700, 5)):       # N runs
        refa[at:at + k] = b"N" * k
    ref = bytes(refa)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    idx = np.asarray(m.mapping.index_map, dtype=np.uint8)
    ref_idx = np.ascontiguousarray(idx[np.frombuffer(ref, dtype=np.uint8)])
    n, cap = 2000, 2000 * 260
    q = np.zeros(cap, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.int64)
    assert model.zsw_model_strand_reads(stable_seed("strands-adversarial"), ref_idx.ctypes.data, len(ref_idx), n, 8, 260, q.ctypes.data, cap, off.ctypes.data) == n
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)[q]
    reads = [letters[off[i]:off[i + 1]].tobytes() for i in range(n)]
    assert min(map(len, reads)) < SEED_MIN_LEN and max(map(len, reads)) > 200
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    F, R = oracle_scores(oracle, sc, reads, ref), oracle_scores(oracle, sc, [rc(x) for x in reads], ref)
    _check_records(za, model, m, -10, -1, reads, ref, F, R)
    assert_result(gpu_strands(za, m, -10, -1, reads, ref), by_contract(F, R), "adversarial reads")


# ---- the tie rule --------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_forward_strand(za, oracle):
    """A reference that holds a 200-base piece and, elsewhere, its reverse complement: a read from the piece scores the same on
    both strands, in either orientation, and the answer is strand 0.
    Counted as scored twice are the reads whose one substitution lies between the sampled k-mers (for 150 bases against 2 kb at
    2/-5, -10/-1 those are columns 1 + 10 j .. 8 + 10 j; columns 9 and 10 stay between them under reversal): every sampled k-mer of
    both orientations occurs, so neither bound falls below the score. An exact copy is different: its score equals the other
    strand's bound, which settles it on the forward strand by the tie rule itself, without a second pass — it is checked for its
    answer only."""
    from zoe_amd import synth

    rng = np.random.default_rng(stable_seed("strands-ties"))
    refa = bytearray(synth.reference_host(2000))
    piece = bytes(refa[300:500])
    refa[1300:1500] = rc(piece)
    ref = bytes(refa)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    ctx = za.SwContext.get(0)
    with_error, exact = [], []
    for i in range(1024):
        at = int(rng.integers(0, 51))
        q = bytearray(piece[at:at + 150])
        exact.append(bytes(q) if i % 2 == 0 else rc(bytes(q)))
        c = 9 + int(rng.integers(0, 2)) + 10 * int(rng.integers(0, 14))
        q[c] = b"ACGT"[(b"ACGT".index(q[c]) + 1 + int(rng.integers(0, 3))) % 4]
        with_error.append(bytes(q) if i % 2 == 0 else rc(bytes(q)))
    for reads, twice in ((with_error, True), (exact, False)):
        want = expected(oracle, sc, reads, ref)
        assert (want[3] == 0).all() and (want[1] == S_).all()
        got = gpu_strands(za, m, -10, -1, reads, ref)
        assert_result(got, want, "ties")
        counts = ctx.strand_counts()
        assert counts[3] == 0
        if twice:
            assert counts == (0, 0, len(reads), 0), counts
        else:  # the score equals the other strand's bound and the forward strand ran first: settled by the tie rule, no second pass
            assert counts == (len(reads), 0, 0, 0), counts


# ---- edge reads ----------------------------------------------------------------------------------------------------------------

def _raw_strands(_lib, lib, h, p: ah.Presented, with_tier: bool = True):
    n = p.rs.n
    out = {k: ah.Out(n, ah.DTYPES[k] if k != "strand" else np.uint8, p.device) for k in ("score", "status", "tier", "strand")}
    rc_ = lib.zsw_score_strands_batch_from(h, p.ref(), 8, 256, out["score"].ptr, out["status"].ptr, out["tier"].ptr if with_tier else None, out["strand"].ptr, None)
    assert rc_ == 0, (rc_, lib.zsw_last_error_string(h).decode())
    if p.device:
        import torch

        torch.cuda.synchronize()
    for k, a in out.items():
        assert a.guards_intact(), f"guard entries around `{k}` were written"
    return out


@pytest.mark.parametrize("pres", ["device-ragged", "host-ragged"])
def test_edge_reads_in_one_ragged_batch(za, oracle, pres):
    """empty reads, reads of 1, 7, 23 and 24 bases, all-N reads, lower-case and IUPAC bytes, a 400-base read; device and host
    memory; the guard entries around every output array stay untouched"""
    from zoe_amd import _lib, synth

    lib = _lib.load()
    rng = np.random.default_rng(stable_seed("strands-edge"))
    ref = synth.reference_host(2000)
    r = np.frombuffer(ref, dtype=np.uint8)
    reads = []
    for rep in range(6):
        for L in (0, 1, 7, 23, 24, 150, 400):
            pos = int(rng.integers(0, len(r) - 400))
            q = r[pos:pos + L].tobytes()
            reads.append(q if rep % 2 == 0 else rc(q))
        reads.append(b"N" * int(rng.integers(1, 200)))
        reads.append(b"n" * 30)
        q = bytearray(r[pos:pos + 150].tobytes().lower() if rep % 2 else r[pos:pos + 150].tobytes())
        for c in rng.integers(0, 150, 10):
            q[c] = b"RYKMSWBDHVNUryu-."[int(rng.integers(0, 17))]
        reads.append(bytes(q) if rep < 3 else rc(bytes(q)))
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    want = expected(oracle, sc, reads, ref)
    assert (want[1] == E_).sum() == 6 and (want[3] == 1).sum() >= 6
    h = ah.new_context(_lib, lib, m, -10, -1, ref)
    try:
        rs = ah.ReadSet("edge", ref, reads, 0, np.zeros(len(reads), dtype=np.int64), np.zeros(len(reads), dtype=np.int64))
        p = ah.Presented(_lib, rs, pres)
        out = _raw_strands(_lib, lib, h, p)
        got = tuple(out[k].data() for k in ("score", "status", "tier", "strand"))
        assert_result(got, want, pres)
        no_tier = _raw_strands(_lib, lib, h, p, with_tier=False)
        assert no_tier["tier"].untouched()
        assert all(np.array_equal(no_tier[k].data(), out[k].data()) for k in ("score", "status", "strand"))
    finally:
        lib.zsw_destroy(h)


# ---- other schemes, another alphabet -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", [(3, -2, -5, 0), (2, -10, -10, -1), (1, -3, -5, -2)], ids=["gap_extend 0", "mismatch loss >= gap_open", "N without potential"])
def test_other_schemes(za, oracle, scheme):
    """1,024 mixed-strand reads (with N in every fourth read: the matrix gives N no potential) through the pruned passes of a small batch"""
    from zoe_amd import _lib, synth

    ma, mi, go, ge = scheme
    ref = synth.reference_host(2000)
    rng = np.random.default_rng(stable_seed("strands-scheme", scheme))
    reads = mixed_strand_reads(ref, 1024, 150, stable_seed("strands-scheme-reads", scheme))
    for i in range(0, 1024, 4):
        q = bytearray(reads[i])
        for c in rng.integers(0, 150, 4):
            q[c:c + 2] = b"NN"[: len(q[c:c + 2])]
        reads[i] = bytes(q)
    ctx = za.SwContext.get(0)
    ctx.debug_set(_lib.DEBUG_SCORE_PRUNE_ANY_SIZE)
    m = za.WeightMatrix.new_dna_matrix(ma, mi, b"N")
    got = gpu_strands(za, m, go, ge, reads, ref)
    assert_result(got, expected(oracle, oracle.dna_scoring(ma, mi, b"N", go, ge), reads, ref), str(scheme))
    counts = ctx.strand_counts()
    assert counts[0] > 0 and counts[1] > 0, counts


def test_25_letter_matrix_scores_every_read_twice(za, oracle):
    """no index for 25 letters: every read is scored on both strands; with an identity complement table rc() is the plain reverse"""
    import torch

    keys = b"ACDEFGHIKLMNPQRSTVWYBJZX*"
    rng = np.random.default_rng(5)
    w = rng.integers(-4, 3, size=(25, 25))
    w = np.minimum(w, w.T)
    np.fill_diagonal(w, rng.integers(4, 12, size=25))
    mp = za.ByteIndexMap.new(keys, b"X")
    pm = za.WeightMatrix.new_custom(mp, w.astype(np.int8))
    alpha = np.frombuffer(keys[:20], dtype=np.uint8)
    pref = rng.choice(alpha, 900).astype(np.uint8)
    n = 256
    start = rng.integers(0, 900 - 120, size=n)
    preads = pref[start[:, None] + np.arange(120)[None, :]].copy()
    preads[rng.random(preads.shape) < 0.04] = alpha[3]
    preads[::7] = rng.choice(alpha, (len(preads[::7]), 120))
    preads[1::2] = preads[1::2, ::-1]  # every other read reversed
    reads = [preads[i].tobytes() for i in range(n)]
    identity = bytes(range(256))
    ctx = za.SwContext.get(0)
    ctx.set_complement(identity)
    sc = oracle.Scoring(w.astype(np.int8), mp.index_map, -11, -1)
    want = expected(oracle, sc, reads, pref.tobytes(), identity)
    assert 0.3 < want[3].mean() < 0.7
    got = gpu_strands(za, pm, -11, -1, reads, pref.tobytes())
    assert_result(got, want, "25 letters")
    assert ctx.strand_counts() == (0, 0, n, int(want[3].sum()))
    torch.cuda.synchronize()


# ---- zsw_orient_batch ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pres", ["device-fixed", "device-ragged", "host-fixed", "host-ragged"])
def test_orient_batch_is_byte_exact(za, pres):
    import torch

    from zoe_amd import _lib, synth

    lib = _lib.load()
    rng = np.random.default_rng(stable_seed("strands-orient", pres))
    ref = synth.reference_host(3000)
    r = np.frombuffer(ref, dtype=np.uint8)
    n = 700
    fixed = pres.endswith("fixed")
    reads = []
    for i in range(n):
        L = 151 if fixed else int(rng.integers(0, 420))
        pos = int(rng.integers(0, len(r) - 420))
        q = bytearray(r[pos:pos + L].tobytes())
        for c in rng.integers(0, max(L, 1), 3 if L else 0):
            q[c] = b"acgtnRYKMSWBDHVN-"[int(rng.integers(0, 17))]
        reads.append(bytes(q))
    strand = rng.integers(0, 2, n).astype(np.uint8)
    want = b"".join(rc(q) if s else q for q, s in zip(reads, strand))
    h = ah.new_context(_lib, lib, za.WeightMatrix.new_dna_matrix(2, -5, b"N"), -10, -1, None)  # neither scoring nor reference is needed
    try:
        rs = ah.ReadSet("orient", ref, reads, 151 if fixed else 0, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
        p = ah.Presented(_lib, rs, pres)
        total = len(want)
        out, back = ah.Out(total, np.uint8, p.device), ah.Out(total, np.uint8, p.device)
        if p.device:
            st = torch.from_numpy(strand).cuda()
            sptr = st.data_ptr()
        else:
            sptr = strand.ctypes.data
        assert lib.zsw_orient_batch(h, p.ref(), sptr, out.ptr, None) == 0, lib.zsw_last_error_string(h).decode()
        if p.device:
            torch.cuda.synchronize()
        assert out.guards_intact()
        assert out.data().tobytes() == want
        # twice with the same strands restores the input (these bytes hold no U, whose complement A does not lead back)
        b2 = _lib.ZswBatch()
        b2.bases, b2.offsets, b2.fixed_len, b2.n_reads, b2.mem, b2.encoding = out.ptr, p.batch.offsets, p.batch.fixed_len, p.batch.n_reads, p.batch.mem, 0
        assert "U" not in want.decode("latin1").upper()
        assert lib.zsw_orient_batch(h, C.byref(b2), sptr, back.ptr, None) == 0
        if p.device:
            torch.cuda.synchronize()
        assert back.guards_intact() and back.data().tobytes() == b"".join(reads)
    finally:
        lib.zsw_destroy(h)


def test_python_mirror_orients_fixed_and_ragged_batches(za):
    """SwContext.orient: byte-exact against Python, the layout of the input kept"""
    import torch

    from zoe_amd import synth

    rng = np.random.default_rng(stable_seed("strands-orient-mirror"))
    ref = synth.reference_host(2000)
    ctx = za.SwContext.get(0)
    for fixed in (True, False):
        reads = [ref[p:p + (150 if fixed else int(rng.integers(1, 300)))] for p in rng.integers(0, 1700, 300)]
        strand = rng.integers(0, 2, len(reads)).astype(np.uint8)
        rb = batch_of(za, reads)
        out = ctx.orient(rb, torch.from_numpy(strand).cuda())
        torch.cuda.synchronize()
        assert (out.fixed_len, out.n_reads, out.offsets is None) == (rb.fixed_len, rb.n_reads, fixed)
        assert out.bases.cpu().numpy().tobytes() == b"".join(rc(q) if s_ else q for q, s_ in zip(reads, strand))


# ---- 3-pass alignment ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("invert", [0, 1])
def test_align_3pass_strands_equals_the_existing_call_on_the_oriented_batch(za, oracle, invert):
    """2,048 mixed-strand reads with indels: every record and ciglet ≡ zsw_align_3pass_batch_from on the oriented batch; strands and
    scores equal the oracle's"""
    from zoe_amd import synth

    ref = synth.reference_host(2000)
    reads = mixed_strand_reads(ref, 2048, 150, stable_seed("strands-align"), rates=(0.02, 0.06, 0.12))
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    want = expected(oracle, sc, reads, ref)
    seq = za.SeqSrc.Query(ref) if invert else za.SeqSrc.Reference(ref)
    got = za.LocalProfilesBatch.new_with_w256(batch_of(za, reads), m, -10, -1).sw_align_strands_from_i8_3pass(seq)
    assert np.array_equal(got.strand, want[3])
    assert np.array_equal(got.status, want[1])
    some = want[1] == S_
    assert np.array_equal(got.records["score"][some], want[0][some])
    assert np.array_equal(got.tier[some], want[2][some])
    oriented = [rc(q) if s else q for q, s in zip(reads, want[3])]
    ex = za.LocalProfilesBatch.new_with_w256(batch_of(za, oriented), m, -10, -1).sw_align_from_i8_3pass(seq)
    assert np.array_equal(got.status, ex.status) and np.array_equal(got.tier, ex.tier)
    assert got.records.tobytes() == ex.records.tobytes()
    assert np.array_equal(got.inc, ex.inc) and np.array_equal(got.op, ex.op)
    gaps = sum(("I" in got.cigar(i) or "D" in got.cigar(i)) for i in range(0, 2048, 8))
    assert gaps > 10  # (not vacuous: a good share of the alignments hold an indel)


# ---- errors, and no state left behind ------------------------------------------------------------------------------------------

def test_errors(za):
    import torch

    from zoe_amd import _lib, synth

    lib = _lib.load()
    ref = synth.reference_host(500)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    reads = [ref[i:i + 60] for i in range(8)]
    rs = ah.ReadSet("err", ref, reads, 60, np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64))
    o = {k: ah.Out(8, np.uint32 if k == "score" else np.uint8, False) for k in ("score", "status", "tier", "strand")}
    h = C.c_void_p()
    assert lib.zsw_create(0, C.byref(h)) == 0
    try:
        p = ah.Presented(_lib, rs, "host-fixed")
        args = lambda strand: (h, p.ref(), 8, 256, o["score"].ptr, o["status"].ptr, o["tier"].ptr, strand, None)
        assert lib.zsw_score_strands_batch_from(*args(o["strand"].ptr)) == -5  # ZSW_ERR_NOT_CONFIGURED
        aln = ah.Out(8, ah.ALN_DTYPE, False)
        total = C.c_uint64(0)
        assert lib.zsw_align_3pass_strands_batch_from(h, p.ref(), 8, 256, 0, aln.ptr, o["status"].ptr, o["tier"].ptr, o["strand"].ptr, None, None, 0,
                                                      C.byref(total), None) == -5
    finally:
        lib.zsw_destroy(h)
    h = ah.new_context(_lib, lib, m, -10, -1, ref)
    try:
        args = lambda strand, pp=p: (h, pp.ref(), 8, 256, o["score"].ptr, o["status"].ptr, o["tier"].ptr, strand, None)
        assert lib.zsw_score_strands_batch_from(*args(None)) == -1  # ZSW_ERR_INVALID_ARGUMENT: out_strand is not optional
        assert lib.zsw_align_3pass_strands_batch_from(h, p.ref(), 8, 256, 0, aln.ptr, o["status"].ptr, o["tier"].ptr, None, None, None, 0, C.byref(total), None) == -1
        packed = ah.Presented(_lib, rs, "host-packed4", lib, h, m.mapping.index_map)
        assert lib.zsw_score_strands_batch_from(*args(o["strand"].ptr, packed)) == -4  # ZSW_ERR_UNSUPPORTED
        assert b"ZSW_ENCODING_BYTES" in lib.zsw_last_error_string(h)
        sb = np.zeros(8, dtype=np.uint8)
        ob = np.zeros(8 * 60, dtype=np.uint8)
        assert lib.zsw_orient_batch(h, packed.ref(), sb.ctypes.data, ob.ctypes.data, None) == -4
        assert all(a.untouched() for a in o.values()) and aln.untouched()
        assert lib.zsw_score_strands_batch_from(*args(o["strand"].ptr)) == 0
        assert (o["strand"].data() == 0).all() and (o["score"].data() == 120).all()
    finally:
        lib.zsw_destroy(h)
    torch.cuda.synchronize()


def test_a_forward_call_after_a_strand_call_returns_what_it_returned_before(za, mixed):
    """no context state leaks: score, ranges and 3-pass alignment of the forward calls, before and after strand calls with another
    complement table"""
    import torch

    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    ctx = za.SwContext.get(0)
    reads = mixed["reads"][:1500]
    ref = mixed["ref"]

    def forward():
        prof = za.LocalProfilesBatch.new_with_w256(batch_of(za, reads), m, -10, -1)
        s = prof.sw_score_from_i8(ref)
        rg = prof.sw_score_ranges_from_i8(za.SeqSrc.Reference(ref))
        al = prof.sw_align_from_i8_3pass(za.SeqSrc.Reference(ref))
        torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in (s.score, s.status, s.tier, rg.score, rg.ref_start, rg.ref_end, rg.query_start, rg.query_end)] + \
               [al.status.tobytes(), al.records.tobytes(), al.inc.tobytes(), al.op.tobytes()], ctx.prune_rescored()

    before = forward()
    ctx.set_complement(bytes(range(256)))
    prof = za.LocalProfilesBatch.new_with_w256(batch_of(za, reads), m, -10, -1)
    prof.sw_score_strands_from_i8(ref)
    prof.sw_align_strands_from_i8_3pass(za.SeqSrc.Reference(ref))
    ctx.set_complement(None)
    prof.sw_score_strands_from_i8(ref)
    assert forward() == before
