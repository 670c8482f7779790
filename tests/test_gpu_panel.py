"""Reference panels (include/zoe_sw.h: zsw_set_panel, zsw_score_panel_batch_from, zsw_panel_gather_batch, zsw_panel_counts).

The contract: R_k = zsw_score_batch_from of the read with member k as the reference; the panel result is R_k of the member that
ranks highest (OVERFLOWED > SOME by score > UNMAPPED = EMPTY), ties to the lowest k, out_ref = that k, everything else bit for bit
what the plain call returns against it. The comparison is always the recipe on the existing code paths — per member
zsw_set_reference + zsw_score_batch_from on the same batch, then rank and lowest k in numpy — and, on a sample of 64 reads per
test, the CPU oracle. The kernel's own values (first choice, supports, bounds) and the counters are pinned to the host model
(tests/models/panel_bound.cpp built as a library), which the CPU suite checks against the full Gotoh matrix."""
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
FORMS = ["device-fixed", "device-ragged", "host-fixed", "host-ragged"]


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


@pytest.fixture(scope="module")
def model():
    d = tempfile.mkdtemp(prefix="zsw_panel_model_")
    so = os.path.join(d, "libpanel_model.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DZSW_MODEL_LIB", "-Wno-unknown-pragmas", "-o", so,
                    os.path.join(ROOT, "tests", "models", "panel_bound.cpp")], check=True)
    lib = C.CDLL(so)
    lib.zsw_model_panel_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]
    lib.zsw_model_panel_todo.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    lib.zsw_model_panel_todo.restype = C.c_ulonglong
    return lib


# ---- members, reads and expected values -----------------------------------------------------------------------------------------

def random_member(seed: int, length: int) -> bytes:
    return ACGT[np.random.default_rng(seed).integers(0, 4, length)].tobytes()


def mutated(rng, r: np.ndarray, n: int, L: int, rate: float) -> list:
    """copies of pieces of `r` with `rate` substitutions and, for a tenth of that per base, single-base indels"""
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


def panel_reads(members: list, n: int, L: int, seed: int, rates=(0.01, 0.05), random_share=0.10, from_members=None) -> list:
    """n reads of L bases: copies of each member (of those at least L + 8 long) at the given divergence rates in equal parts, a
    share of random reads, an N or three in every eighth read; shuffled"""
    rng = np.random.default_rng(seed)
    src = [np.frombuffer(m, dtype=np.uint8) for k, m in enumerate(members) if len(m) >= L + 16 and (from_members is None or k in from_members)]
    n_random = int(round(n * random_share))
    cells = [(r, rate) for r in src for rate in rates]
    per = (n - n_random) // len(cells)
    reads = []
    for c, (r, rate) in enumerate(cells):
        reads += mutated(rng, r, per if c + 1 < len(cells) else n - n_random - per * (len(cells) - 1), L, rate)
    reads += [ACGT[rng.integers(0, 4, L)].tobytes() for _ in range(n_random)]
    reads = [reads[i] for i in rng.permutation(n)]
    for i in range(0, n, 8):
        q = bytearray(reads[i])
        for c in rng.integers(0, L, int(rng.integers(1, 4))):
            q[c] = ord("N")
        reads[i] = bytes(q)
    return reads


def rank(score, status):
    score, status = np.asarray(score, dtype=np.uint64), np.asarray(status)
    return np.where(status == O_, np.uint64(2) << np.uint64(32), np.where(status == S_, (np.uint64(1) << np.uint64(32)) | score, np.uint64(0)))


def by_contract(per_member: list):
    """(score, status, tier, ref) of the contract from the members' (score, status, tier): the highest rank, the lowest member"""
    ranks = np.stack([rank(m[0], m[1]) for m in per_member])
    ref = np.argmax(ranks, axis=0).astype(np.uint32)  # the first maximum
    pick = lambda k: np.stack([np.asarray(m[k]) for m in per_member])[ref, np.arange(len(ref))]
    return pick(0), pick(1), pick(2), ref


class Ctx:
    """a context of its own over the raw C ABI, with the scoring of `matrix`"""

    def __init__(self, za, matrix, go: int, ge: int):
        from zoe_amd import _lib

        self._lib, self.lib = _lib, _lib.load()
        self.h = ah.new_context(_lib, self.lib, matrix, go, ge, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import torch

        torch.cuda.synchronize()
        self.lib.zsw_destroy(self.h)

    def err(self) -> str:
        return self.lib.zsw_last_error_string(self.h).decode()

    def set_panel(self, members: list) -> int:
        cat = np.frombuffer(b"".join(members) or b"\0", dtype=np.uint8)
        off = np.zeros(len(members) + 1, dtype=np.uint64)
        np.cumsum([len(m) for m in members], out=off[1:])
        return self.lib.zsw_set_panel(self.h, cat.ctypes.data, off.ctypes.data, len(members), self._lib.MEM_HOST)

    def present(self, reads: list, form: str) -> ah.Presented:
        lens = {len(q) for q in reads}
        fixed = len(lens) == 1 and 0 not in lens
        rs = ah.ReadSet("panel", b"", reads, len(reads[0]) if fixed else 0, np.zeros(len(reads), dtype=np.int64), np.zeros(len(reads), dtype=np.int64))
        return ah.Presented(self._lib, rs, form)

    def panel(self, p: ah.Presented, width: int = 8, with_tier: bool = True):
        """zsw_score_panel_batch_from with guarded outputs -> (score, status, tier, ref)"""
        import torch

        n = p.rs.n
        out = {k: ah.Out(n, np.uint32 if k in ("score", "ref") else np.uint8, p.device) for k in ("score", "status", "tier", "ref")}
        rc = self.lib.zsw_score_panel_batch_from(self.h, p.ref(), width, 256, out["score"].ptr, out["status"].ptr, out["tier"].ptr if with_tier else None,
                                                 out["ref"].ptr, None)
        assert rc == 0, (rc, self.err())
        torch.cuda.synchronize()
        for k, a in out.items():
            assert a.guards_intact(), f"guard entries around `{k}` were written"
        if not with_tier:
            assert out["tier"].untouched()
        return tuple(out[k].data() for k in ("score", "status", "tier", "ref"))

    def plain(self, p: ah.Presented, member: bytes, width: int = 8):
        """the parent's code path: zsw_set_reference + zsw_score_batch_from -> (score, status, tier)"""
        import torch

        r = np.frombuffer(member, dtype=np.uint8)
        assert self.lib.zsw_set_reference(self.h, r.ctypes.data, len(member), self._lib.MEM_HOST) == 0
        n = p.rs.n
        out = {k: ah.Out(n, np.uint32 if k == "score" else np.uint8, p.device) for k in ("score", "status", "tier")}
        rc = self.lib.zsw_score_batch_from(self.h, p.ref(), width, 256, out["score"].ptr, out["status"].ptr, out["tier"].ptr, None)
        assert rc == 0, (rc, self.err())
        torch.cuda.synchronize()
        return tuple(out[k].data() for k in ("score", "status", "tier"))

    def recipe(self, p: ah.Presented, members: list, width: int = 8):
        per = [self.plain(p, m, width) for m in members]
        return by_contract(per), per

    def counts(self):
        c = (C.c_uint64 * 4)()
        assert self.lib.zsw_panel_counts(self.h, c) == 0
        return tuple(int(x) for x in c)

    def pruning(self, on: bool):
        assert self.lib.zsw_set_option(self.h, self._lib.OPTION_EXACT_PRUNING, 1 if on else 0) == 0

    def debug(self, flags: int):
        assert self.lib.zsw_debug_set(self.h, flags) == 0


def assert_result(got, want, what: str):
    for k, name in ((1, "status"), (0, "score"), (3, "ref"), (2, "tier")):
        bad = np.nonzero(got[k] != want[k])[0]
        assert not len(bad), f"{what}: `{name}` differs at {len(bad)} reads, first {list(bad[:5])}: got {got[k][bad[:5]]}, want {want[k][bad[:5]]}"


def oracle_check(o, sc, reads: list, members: list, got, width: int = 8, size: int = 64):
    """the contract from the CPU oracle on an evenly spaced sample of the reads (score, status, member; the tier where there is a score)"""
    idx = np.unique(np.linspace(0, len(reads) - 1, min(size, len(reads))).astype(np.int64))
    idx = np.array([i for i in idx if len(reads[i]) > 0], dtype=np.int64)
    sample = [reads[i] for i in idx]
    off = np.zeros(len(sample) + 1, dtype=np.uint64)
    np.cumsum([len(q) for q in sample], out=off[1:])
    cat = np.frombuffer(b"".join(sample), dtype=np.uint8)
    per = [o.batch_score_w256(width, sc, cat, m, offsets=off, threads=ah.ORACLE_THREADS) for m in members]
    want = by_contract(per)
    for k, name in ((1, "status"), (0, "score"), (3, "ref")):
        assert np.array_equal(got[k][idx], want[k]), f"oracle: `{name}` differs: got {got[k][idx]}, want {want[k]}"
    some = want[1] == S_
    assert np.array_equal(got[2][idx][some], want[2][some]), "oracle: tiers differ"


@pytest.fixture(scope="module")
def trio():
    """the panel of the first tests — 300, 2,000 and 2,100 random bases, so that both k-mer lengths occur — and its 4,096 reads"""
    members = [random_member(stable_seed("panel-member", k), L) for k, L in enumerate((300, 2000, 2100))]
    return {"members": members, "reads": panel_reads(members, 4096, 150, stable_seed("panel-reads"))}


@pytest.fixture(scope="module")
def dna(za):
    return za.WeightMatrix.new_dna_matrix(2, -5, b"N")


# ---- equality with the recipe ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_equals_the_recipe_in_all_four_forms_with_and_without_the_proof(za, oracle, dna, trio, form):
    """4,096 reads of 150 bases: copies of each member at 1 % + 0.1 % and 5 % + 0.5 %, 10 % random reads, reads with N"""
    members, reads = trio["members"], trio["reads"]
    with Ctx(za, dna, -10, -1) as c:
        assert c.set_panel(members) == 0, c.err()
        p = c.present(reads, form)
        want, per = c.recipe(p, members)
        assert len(set(want[3])) == 3 and (want[1] == S_).mean() > 0.95
        got = c.panel(p)
        assert_result(got, want, f"{form}, exact pruning on")
        on = c.counts()
        assert on[1] == 4096 and on[0] > 2000 and on[1] + on[2] < 3 * 4096, on  # (not vacuous: most reads are settled after one score)
        oracle_check(oracle, oracle.dna_scoring(2, -5, b"N", -10, -1), reads, members, got)
        no_tier = c.panel(p, with_tier=False)
        assert all(np.array_equal(no_tier[k], got[k]) for k in (0, 1, 3))
        c.pruning(False)
        off = c.panel(p)
        assert_result(off, want, f"{form}, exact pruning off")
        assert c.counts() == (0, 4096, 2 * 4096, 4096)


@pytest.mark.parametrize("width", [16, 32])
def test_equals_the_recipe_from_every_width(za, oracle, dna, trio, width):
    members, reads = trio["members"], trio["reads"]
    with Ctx(za, dna, -10, -1) as c:
        assert c.set_panel(members) == 0
        p = c.present(reads, "device-fixed")
        want, _ = c.recipe(p, members, width)
        got = c.panel(p, width)
        assert (got[2] == width).all()
        assert_result(got, want, f"from i{width}")
        oracle_check(oracle, oracle.dna_scoring(2, -5, b"N", -10, -1), reads, members, got, width)


def test_equals_the_recipe_on_a_small_batch_through_the_pruned_passes(za, oracle, dna, trio):
    """300 reads under ZSW_DEBUG_SCORE_PRUNE_ANY_SIZE: every group, however small, takes the seeded pass"""
    from zoe_amd import _lib

    members, reads = trio["members"], trio["reads"][:300]
    with Ctx(za, dna, -10, -1) as c:
        c.debug(_lib.DEBUG_SCORE_PRUNE_ANY_SIZE)
        assert c.set_panel(members) == 0
        for form in ("device-fixed", "host-ragged"):
            p = c.present(reads, form)
            want, _ = c.recipe(p, members)
            got = c.panel(p)
            assert_result(got, want, form)
        oracle_check(oracle, oracle.dna_scoring(2, -5, b"N", -10, -1), reads, members, got)


# ---- ties ------------------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_lowest_member(za, oracle, dna):
    """Identical members at 0 and 2: member 0 answers every read of theirs. The identical pair at 1 and 2: member 1 answers
    wherever the pair wins. Exact copies: the score equals the bound of the other copy, which the tie clause rules out for the
    higher member — every such read is settled after one score."""
    a, b = random_member(stable_seed("panel-tie", 0), 2000), random_member(stable_seed("panel-tie", 1), 1200)
    ra = np.frombuffer(a, dtype=np.uint8)
    rng = np.random.default_rng(stable_seed("panel-tie-reads"))
    exact = [a[s:s + 150] for s in rng.integers(0, 1850, 1024)]
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    with Ctx(za, dna, -10, -1) as c:
        for members, winner in (([a, b, a], 0), ([b, a, a], 1)):
            assert c.set_panel(members) == 0
            from_a = mutated(rng, ra, 1024, 150, 0.03)
            mixed = panel_reads(members, 2048, 150, stable_seed("panel-tie-mixed", winner), rates=(0.02, 0.06))
            for reads, what in ((from_a, "copies of the pair"), (mixed, "mixed"), (exact, "exact copies")):
                p = c.present(reads, "device-fixed")
                want, per = c.recipe(p, members)
                got = c.panel(p)
                assert_result(got, want, what)
                assert not (got[3] == 2).any()
                if reads is not mixed:
                    assert (got[3] == winner).all()
                    assert np.array_equal(per[winner][0], per[2][0])  # (the pair does tie)
                if reads is exact:
                    assert (got[0] == 300).all()
                    assert c.counts() == (1024, 1024, 0, 0), c.counts()
            oracle_check(oracle, sc, mixed, members, c.panel(c.present(mixed, "device-fixed")))


# ---- edge reads ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["device-ragged", "host-ragged"])
def test_edge_reads_in_one_ragged_batch(za, oracle, dna, trio, form):
    """empty reads (EMPTY, member 0), reads of 1, 23, 24 and 25 bases around SEED_MIN_LEN, a 400-base read — longer than the
    shortest member —, all-N reads (UNMAPPED, member 0), lower-case and IUPAC bytes"""
    members = trio["members"]
    rng = np.random.default_rng(stable_seed("panel-edge"))
    reads = []
    for rep in range(8):
        r = np.frombuffer(members[rep % 3], dtype=np.uint8)
        for L in (0, 1, 23, 24, 25, 150, 400):
            L = min(L, len(r))
            pos = int(rng.integers(0, len(r) - L + 1))
            reads.append(r[pos:pos + L].tobytes())
        reads.append(np.frombuffer(members[1], dtype=np.uint8)[100:500].tobytes())  # 400 bases against the 300-base member too
        reads.append(b"N" * int(rng.integers(1, 200)))
        q = bytearray(r[:150].tobytes().lower() if rep % 2 else r[:150].tobytes())
        for cc in rng.integers(0, 150, 10):
            q[cc] = b"RYKMSWBDHVNUryu-."[int(rng.integers(0, 17))]
        reads.append(bytes(q))
    with Ctx(za, dna, -10, -1) as c:
        assert c.set_panel(members) == 0
        p = c.present(reads, form)
        want, _ = c.recipe(p, members)
        got = c.panel(p)
        assert_result(got, want, form)
        empty = np.array([len(q) == 0 for q in reads])
        all_n = np.array([len(q) > 0 and set(q) == {ord("N")} for q in reads])
        assert empty.sum() == 8 and (got[1][empty] == E_).all() and (got[3][empty] == 0).all()
        assert all_n.sum() == 8 and (got[1][all_n] == U_).all() and (got[3][all_n] == 0).all()
        assert len(set(got[3])) == 3
        oracle_check(oracle, oracle.dna_scoring(2, -5, b"N", -10, -1), reads, members, got)


# ---- one member, sixty-four members ----------------------------------------------------------------------------------------------

def test_one_member_is_the_plain_call(za, dna, trio):
    member, reads = trio["members"][1], trio["reads"]
    with Ctx(za, dna, -10, -1) as c:
        assert c.set_panel([member]) == 0
        for form in ("device-fixed", "host-ragged"):
            p = c.present(reads, form)
            plain = c.plain(p, member)
            got = c.panel(p)
            assert all(np.array_equal(got[k], plain[k]) for k in range(3)) and (got[3] == 0).all()
            assert c.counts() == (4096, 4096, 0, 4096)


def test_sixty_four_members(za, oracle, dna):
    """64 members of 64 to 200 bases, 1,024 reads of 60 bases"""
    rng = np.random.default_rng(stable_seed("panel-64"))
    members = [random_member(stable_seed("panel-64-member", k), int(rng.integers(64, 201))) for k in range(64)]
    reads = panel_reads(members, 1024, 60, stable_seed("panel-64-reads"), rates=(0.01, 0.05))
    with Ctx(za, dna, -10, -1) as c:
        assert c.set_panel(members) == 0, c.err()
        p = c.present(reads, "device-fixed")
        want, _ = c.recipe(p, members)
        assert len(set(want[3])) > 40
        got = c.panel(p)
        assert_result(got, want, "64 members")
        cnt = c.counts()
        assert cnt[1] == 1024 and cnt[1] + cnt[2] < 64 * 1024, cnt
        oracle_check(oracle, oracle.dna_scoring(2, -5, b"N", -10, -1), reads, members, got)


# ---- other schemes, another alphabet ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", [(3, -2, -5, 0), (2, -10, -10, -1), (1, -3, -5, -2)], ids=["gap_extend 0", "mismatch loss >= gap_open", "N without potential"])
def test_other_schemes(za, oracle, trio, scheme):
    """1,024 reads (with N in every eighth read: the matrix gives N no potential) through the pruned passes of small groups"""
    from zoe_amd import _lib

    ma, mi, go, ge = scheme
    members = trio["members"]
    reads = panel_reads(members, 1024, 150, stable_seed("panel-scheme", scheme))
    with Ctx(za, za.WeightMatrix.new_dna_matrix(ma, mi, b"N"), go, ge) as c:
        c.debug(_lib.DEBUG_SCORE_PRUNE_ANY_SIZE)
        assert c.set_panel(members) == 0
        p = c.present(reads, "device-fixed")
        want, _ = c.recipe(p, members)
        got = c.panel(p)
        assert_result(got, want, str(scheme))
        assert c.counts()[0] > 0
        oracle_check(oracle, oracle.dna_scoring(ma, mi, b"N", go, ge), reads, members, got)


def test_25_letter_matrix_scores_every_read_against_every_member(za, oracle):
    """no index for 25 letters: no member has a bound, member 0 runs first and every read is scored against all of them"""
    keys = b"ACDEFGHIKLMNPQRSTVWYBJZX*"
    rng = np.random.default_rng(5)
    w = rng.integers(-4, 3, size=(25, 25))
    w = np.minimum(w, w.T)
    np.fill_diagonal(w, rng.integers(4, 12, size=25))
    mp = za.ByteIndexMap.new(keys, b"X")
    pm = za.WeightMatrix.new_custom(mp, w.astype(np.int8))
    alpha = np.frombuffer(keys[:20], dtype=np.uint8)
    members = [rng.choice(alpha, L).astype(np.uint8).tobytes() for L in (500, 900, 700)]
    n = 256
    reads = []
    for i in range(n):
        m = np.frombuffer(members[i % 3], dtype=np.uint8)
        s = int(rng.integers(0, len(m) - 120))
        q = m[s:s + 120].copy()
        q[rng.random(120) < 0.04] = alpha[3]
        reads.append((rng.choice(alpha, 120).astype(np.uint8) if i % 7 == 0 else q).tobytes())
    with Ctx(za, pm, -11, -1) as c:
        assert c.set_panel(members) == 0
        p = c.present(reads, "device-fixed")
        want, _ = c.recipe(p, members)
        assert len(set(want[3])) == 3
        got = c.panel(p)
        assert_result(got, want, "25 letters")
        assert c.counts() == (0, n, 2 * n, n)
        oracle_check(oracle, oracle.Scoring(w.astype(np.int8), mp.index_map, -11, -1), reads, members, got)


# ---- the kernel pinned to the model ----------------------------------------------------------------------------------------------

def _model_records(model, matrix, go, ge, members: list, reads: list):
    n, K = len(reads), len(members)
    w = np.ascontiguousarray(matrix.signed_weights().astype(np.int32))
    idx = np.asarray(matrix.mapping.index_map, dtype=np.uint8)
    refs = np.ascontiguousarray(idx[np.frombuffer(b"".join(members), dtype=np.uint8)])
    roff = np.zeros(K + 1, dtype=np.int64)
    np.cumsum([len(m) for m in members], out=roff[1:])
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(q) for q in reads], out=off[1:])
    q_idx = np.ascontiguousarray(idx[np.frombuffer(b"".join(reads) or b"\0", dtype=np.uint8)])
    out = np.zeros((n, 2 + 2 * K), dtype=np.int32)
    usable = model.zsw_model_panel_batch(w.ctypes.data, w.shape[0], -go, -ge, refs.ctypes.data, roff.ctypes.data, K, q_idx.ctypes.data, off.ctypes.data, n,
                                         SEED_TOL, SEED_MIN_LEN, out.ctypes.data)
    return out, usable


def _check_records(za, model, c: "Ctx", matrix, go, ge, members: list, reads: list, form: str):
    """every int of zsw_debug_panel_records against the model, and zsw_panel_counts against the model's rule applied to the scores
    of the plain calls; returns the counters"""
    import torch

    n, K = len(reads), len(members)
    p = c.present(reads, form)
    _, per = c.recipe(p, members)
    rec = torch.full((n, 2 + 2 * K), -7, dtype=torch.int32, device="cuda")
    assert c.lib.zsw_debug_panel_records(c.h, C.c_void_p(rec.data_ptr())) == 0
    try:
        c.panel(p)
    finally:
        assert c.lib.zsw_debug_panel_records(c.h, None) == 0
    rec = rec.cpu().numpy()
    counts = c.counts()
    out, usable = _model_records(model, matrix, go, ge, members, reads)
    assert usable == K
    first = out[:, 0]
    todo = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        sp, st = per[first[i]][0][i], per[first[i]][1][i]
        b = np.ascontiguousarray(out[i, 2 + K:])
        todo[i] = model.zsw_model_panel_todo(K, int(first[i]), int(st == S_), int(sp), b.ctypes.data)
    out[:, 1] = todo == 0
    bad = np.nonzero((rec != out).any(axis=1))[0]
    assert not len(bad), f"{len(bad)} reads differ, first: {[(int(i), rec[i].tolist(), out[i].tolist()) for i in bad[:5]]} (kernel, model)"
    listed = np.array([bin(int(t)).count("1") for t in todo])
    assert counts == (int((todo == 0).sum()), n, int(listed.sum()), int((listed == K - 1).sum())), counts
    return counts


def test_kernel_values_and_counters_equal_the_model(za, model, dna, trio):
    members, reads = trio["members"], trio["reads"]
    with Ctx(za, dna, -10, -1) as c:
        assert c.set_panel(members) == 0
        counts = _check_records(za, model, c, dna, -10, -1, members, reads, "device-fixed")
        assert counts[0] > 2000  # (not vacuous)
        near = panel_reads(members, 2048, 150, stable_seed("panel-near"), rates=(0.01,), random_share=0.0)
        counts = _check_records(za, model, c, dna, -10, -1, members, near, "device-fixed")
        assert counts[1] + counts[2] < 3 * 2048 and counts[0] > 1500, counts  # the 1 % set: far fewer than K * n pairs are scored
        c.pruning(False)
        c.panel(c.present(near, "device-fixed"))
        assert c.counts()[1] + c.counts()[2] == 3 * 2048


def test_kernel_values_equal_the_model_on_ragged_reads(za, model, dna, trio):
    """reads of 1 to 260 bases, through the kernel that reads its bases from global memory"""
    members = trio["members"]
    rng = np.random.default_rng(stable_seed("panel-ragged"))
    reads = []
    for i in range(1500):
        r = np.frombuffer(members[i % 3], dtype=np.uint8)
        L = int(rng.integers(1, 261))
        reads.append(mutated(rng, r, 1, L, 0.03)[0] if L > 40 else r[:L].tobytes() if i % 2 else ACGT[rng.integers(0, 4, L)].tobytes())
    with Ctx(za, dna, -10, -1) as c:
        assert c.set_panel(members) == 0
        _check_records(za, model, c, dna, -10, -1, members, reads, "device-ragged")


# ---- zsw_panel_gather_batch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_gather_is_byte_exact(za, dna, form):
    import torch

    rng = np.random.default_rng(stable_seed("panel-gather", form))
    fixed = form.endswith("fixed")
    n = 700
    reads = [ACGT[rng.integers(0, 4, 151 if fixed else int(rng.integers(0, 420)))].tobytes() for _ in range(n)]
    with Ctx(za, dna, -10, -1) as c:  # neither scoring nor panel is needed
        p = c.present(reads, form)
        total = sum(len(q) for q in reads)
        for ref_of, k in ((rng.integers(0, 3, n), 5), (rng.integers(0, 3, n), 1), (np.full(n, 2), 2)):  # no reads, some reads, all reads
            ref_of = ref_of.astype(np.uint32)
            picked = [i for i in range(n) if ref_of[i] == k]
            bases, index, offs = ah.Out(max(total, 1), np.uint8, p.device), ah.Out(n, np.uint32, p.device), ah.Out(n + 1, np.uint64, p.device)
            if p.device:
                t = torch.from_numpy(ref_of.view(np.int32)).cuda()
                rptr = t.data_ptr()
            else:
                rptr = ref_of.ctypes.data
            m = C.c_uint64(123)
            rc = c.lib.zsw_panel_gather_batch(c.h, p.ref(), rptr, k, bases.ptr, None if fixed else offs.ptr, index.ptr, C.byref(m), None)
            assert rc == 0, (rc, c.err())
            torch.cuda.synchronize()
            assert m.value == len(picked)
            assert bases.guards_intact() and index.guards_intact() and offs.guards_intact()
            want = b"".join(reads[i] for i in picked)
            assert bases.data()[:len(want)].tobytes() == want
            assert index.data()[:len(picked)].tolist() == picked
            if fixed:
                assert offs.untouched()
            else:
                assert offs.data()[:len(picked) + 1].tolist() == np.concatenate([[0], np.cumsum([len(reads[i]) for i in picked])]).astype(np.int64).tolist()


def test_python_mirror_gathers_and_the_3pass_call_runs_on_the_group(za, dna, trio):
    """SwContext.set_panel / sw_score_panel_from_i8 / panel_gather; then per member set_reference + the 3-pass call on its gathered
    group equals the 3-pass call on the same reads picked out by hand"""
    import torch

    members, reads = trio["members"], trio["reads"][:1500]
    ctx = za.SwContext.get(0)
    assert ctx.set_panel(members) == 3
    for fixed in (True, False):
        rs = reads if fixed else [q[:100 + i % 50] for i, q in enumerate(reads)]
        rb = za.ReadBatch.from_sequences(rs)
        got = za.LocalProfilesBatch.new_with_w256(rb, dna, -10, -1).sw_score_panel_from_i8()
        torch.cuda.synchronize()
        ref = got.ref.cpu().numpy()
        assert len(set(ref)) == 3
        for k in range(3):
            group, index = ctx.panel_gather(rb, got.ref, k)
            torch.cuda.synchronize()
            picked = np.nonzero(ref == k)[0]
            assert np.array_equal(index.cpu().numpy(), picked) and group.n_reads == len(picked)
            assert (group.fixed_len, group.offsets is None) == (rb.fixed_len, fixed)
            by_hand = [rs[i] for i in picked]
            assert group.bases.cpu().numpy()[:sum(map(len, by_hand))].tobytes() == b"".join(by_hand)
            seq = za.SeqSrc.Reference(members[k])
            a = za.LocalProfilesBatch.new_with_w256(group, dna, -10, -1).sw_align_from_i8_3pass(seq)
            b = za.LocalProfilesBatch.new_with_w256(za.ReadBatch.from_sequences(by_hand), dna, -10, -1).sw_align_from_i8_3pass(seq)
            assert a.records.tobytes() == b.records.tobytes() and np.array_equal(a.status, b.status)
            assert np.array_equal(a.inc, b.inc) and np.array_equal(a.op, b.op)
            score = got.score.cpu().numpy()[picked]
            some = a.status == S_
            assert np.array_equal(a.records["score"][some], score.view(np.uint32)[some])


def test_set_panel_from_a_device_fasta_batch(za, dna, trio):
    """fasta_batch_from_text -> set_panel, device to device: the same results as from host byte strings"""
    import torch

    from zoe_amd import records

    members, reads = trio["members"], trio["reads"][:2048]
    text = b"".join(b">m%d some text\n" % k + b"\n".join(m[i:i + 70] for i in range(0, len(m), 70)) + b"\n" for k, m in enumerate(members))
    ctx = za.SwContext.get(0)
    prof = za.LocalProfilesBatch.new_with_w256(za.ReadBatch.from_sequences(reads), dna, -10, -1)
    assert ctx.set_panel(members) == 3
    a = prof.sw_score_panel_from_i8()
    fb = records.fasta_batch_from_text(text)
    assert ctx.set_panel(fb) == 3
    b = prof.sw_score_panel_from_i8()
    torch.cuda.synchronize()
    for name in ("score", "status", "tier", "ref"):
        assert np.array_equal(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), name
    assert len(set(a.ref.cpu().numpy())) == 3


# ---- errors, and no state left behind --------------------------------------------------------------------------------------------

def test_errors(za, dna, trio):
    import torch

    from zoe_amd import _lib

    lib = _lib.load()
    members = trio["members"]
    reads = [members[1][i:i + 60] for i in range(8)]
    o = {k: ah.Out(8, np.uint32 if k in ("score", "ref") else np.uint8, False) for k in ("score", "status", "tier", "ref")}
    cat = np.frombuffer(b"".join(members), dtype=np.uint8)
    off = np.array([0, 300, 2300, 4400], dtype=np.uint64)
    h = C.c_void_p()
    assert lib.zsw_create(0, C.byref(h)) == 0
    try:  # no scoring, then no panel
        rs = ah.ReadSet("err", b"", reads, 60, np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64))
        p = ah.Presented(_lib, rs, "host-fixed")
        args = lambda ref, pp=p, hh=h: (hh, pp.ref(), 8, 256, o["score"].ptr, o["status"].ptr, o["tier"].ptr, ref, None)
        assert lib.zsw_set_panel(h, cat.ctypes.data, off.ctypes.data, 3, _lib.MEM_HOST) == 0
        assert lib.zsw_score_panel_batch_from(*args(o["ref"].ptr)) == -5  # ZSW_ERR_NOT_CONFIGURED: no scoring
    finally:
        lib.zsw_destroy(h)
    with Ctx(za, dna, -10, -1) as c:
        h = c.h
        args = lambda ref, pp=p: (h, pp.ref(), 8, 256, o["score"].ptr, o["status"].ptr, o["tier"].ptr, ref, None)
        assert lib.zsw_score_panel_batch_from(*args(o["ref"].ptr)) == -5  # no panel
        assert lib.zsw_set_panel(h, cat.ctypes.data, off.ctypes.data, 0, _lib.MEM_HOST) == -1
        off65 = np.arange(66, dtype=np.uint64)
        assert lib.zsw_set_panel(h, cat.ctypes.data, off65.ctypes.data, 65, _lib.MEM_HOST) == -1
        assert lib.zsw_set_panel(h, cat.ctypes.data, np.array([0, 300, 300, 4400], dtype=np.uint64).ctypes.data, 3, _lib.MEM_HOST) == 1  # ZSW_ERR_EMPTY_SEQUENCE
        assert lib.zsw_set_panel(h, cat.ctypes.data, np.array([0, 2300, 300, 4400], dtype=np.uint64).ctypes.data, 3, _lib.MEM_HOST) == -1
        assert b"monotone" in lib.zsw_last_error_string(h)
        assert lib.zsw_score_panel_batch_from(*args(o["ref"].ptr)) == -5  # the failed calls have set nothing
        assert lib.zsw_set_panel(h, cat.ctypes.data, off.ctypes.data, 3, _lib.MEM_HOST) == 0
        assert lib.zsw_score_panel_batch_from(*args(None)) == -1  # out_ref is not optional
        packed = ah.Presented(_lib, rs, "host-packed4", lib, h, dna.mapping.index_map)
        assert lib.zsw_score_panel_batch_from(*args(o["ref"].ptr, packed)) == -4  # ZSW_ERR_UNSUPPORTED
        gi, gm = np.zeros(8, dtype=np.uint32), C.c_uint64(0)
        assert lib.zsw_panel_gather_batch(h, packed.ref(), gi.ctypes.data, 0, np.zeros(480, dtype=np.uint8).ctypes.data, None, gi.ctypes.data, C.byref(gm), None) == -4
        assert lib.zsw_set_option(h, _lib.OPTION_MIN_SCORE, 50) == 0
        assert lib.zsw_score_panel_batch_from(*args(o["ref"].ptr)) == -4
        assert b"ZSW_OPTION_MIN_SCORE" in lib.zsw_last_error_string(h)
        assert lib.zsw_set_option(h, _lib.OPTION_MIN_SCORE, 0) == 0
        assert all(a.untouched() for a in o.values())
        assert lib.zsw_score_panel_batch_from(*args(o["ref"].ptr)) == 0, c.err()
        assert (o["ref"].data() == 1).all() and (o["score"].data() == 120).all()
    torch.cuda.synchronize()


def test_set_scoring_after_set_panel_rebuilds_the_indices(za, oracle, trio):
    members, reads = trio["members"], trio["reads"]
    with Ctx(za, za.WeightMatrix.new_dna_matrix(2, -5, b"N"), -10, -1) as c:
        assert c.set_panel(members) == 0
        p = c.present(reads, "device-fixed")
        c.panel(p)  # builds the indices under 2/-5
        m2 = za.WeightMatrix.new_dna_matrix(3, -4, b"N")
        w = np.ascontiguousarray(m2.signed_weights(), dtype=np.int8)
        im = np.ascontiguousarray(m2.mapping.index_map, dtype=np.uint8)
        assert c.lib.zsw_set_scoring(c.h, w.ctypes.data, w.shape[0], im.ctypes.data, -6, -2) == 0
        want, _ = c.recipe(p, members)
        got = c.panel(p)
        assert_result(got, want, "after zsw_set_scoring")
        assert c.counts()[0] > 2000
        oracle_check(oracle, oracle.dna_scoring(3, -4, b"N", -6, -2), reads, members, got)


def test_neighbours(za, dna, trio):
    """a plain call after a panel call returns what it returned before; two panel calls in a row return the same arrays"""
    members, reads = trio["members"], trio["reads"]
    with Ctx(za, dna, -10, -1) as c:
        p = c.present(reads, "device-fixed")
        before = c.plain(p, members[2])
        assert c.set_panel(members) == 0
        a = c.panel(p)
        b = c.panel(p)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        n = p.rs.n
        out = {k: ah.Out(n, np.uint32 if k == "score" else np.uint8, True) for k in ("score", "status", "tier")}
        assert c.lib.zsw_score_batch_from(c.h, p.ref(), 8, 256, out["score"].ptr, out["status"].ptr, out["tier"].ptr, None) == 0  # the reference is still member 2
        import torch

        torch.cuda.synchronize()
        assert all(np.array_equal(out[k].data(), before[i]) for i, k in enumerate(("score", "status", "tier")))
