"""The alignment certificates as shipped: the kernel's own verdicts against zsw_cert.hpp compiled for the host.

By default most sw_simd_align CIGARs come from the certificate mode of the classify pass (zoe_amd/csrc/zsw_threepass.hip; the
decision is zoe_amd/csrc/zsw_cert.hpp), not from the striped recurrence. Here the kernel reports its verdict per read
(zsw_debug_cert_records), and tests/models/align_onegap_cert.cpp, built as a library, recomputes it from the read and the kernel's
first-pass values with the same header — the CPU suite checks that header against counting Gotoh and the literal sw_simd_align. Per
configuration (both roles, seven schemes on which the certificate must engage, one that the seeded pass refuses, i16 / u16 / i32 and
8-bit lanes on short reads at the overflow limit): every record, status, tier and ciglet equals the all-literal path
(ZSW_DEBUG_ALIGN_NO_CERTIFICATE); the kernel's records equal the host verdicts on every read; a sample of reads flagged unique has
unique maxima at the reported corners (plain Gotoh), and the certified ones exactly the certified optimal alignments between them;
the oracle's literal sw_simd_align agrees on a sample; gapless and one-gap certificates meet a floor, so that no check is vacuous."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, stable_seed

pytestmark = pytest.mark.gpu

NOT_UNIQUE, GAPLESS, ONE_GAP, DIAG_SUM, POTENTIAL, TWO_RUNS, PLACEMENT, DEFERRED = range(8)  # zsw_cert.hpp CertVerdict
UNSET = -7


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


@pytest.fixture(scope="module")
def model():
    d = tempfile.mkdtemp(prefix="zsw_cert_model_")
    so = os.path.join(d, "libcert_model.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DZSW_MODEL_LIB", "-Wno-unknown-pragmas", "-o", so,
                    os.path.join(ROOT, "tests", "models", "align_onegap_cert.cpp")], check=True)
    lib = C.CDLL(so)
    vp, i, u = C.c_void_p, C.c_int, C.c_uint32
    lib.zsw_model_cert_verdicts.argtypes = [vp, i, i, i, vp, u, vp, vp, u, i, vp, vp, vp, vp, vp, vp, vp]
    lib.zsw_model_cert_verdicts.restype = i
    lib.zsw_model_cert_corners.argtypes = [vp, i, i, i, vp, u, vp, vp, u, i, vp, vp]
    lib.zsw_model_cert_corners.restype = i
    return lib


def _matrices(za):
    """name -> (matrix, gap_open, gap_extend, alphabet, engages): the certificate must engage on all but the last"""
    dna = za.WeightMatrix.new_dna_matrix
    asym = za.WeightMatrix.new_custom(za.alignment.DNA_PROFILE_MAP, [[4, -3, -2, -5, 0], [-1, 4, -4, -2, 0], [-3, -2, 4, -1, 0],
                                                                    [-4, -5, -1, 4, 0], [0, 0, 0, 0, 0]])
    acg = za.WeightMatrix.new(za.ByteIndexMap.new(b"ACG", b"A"), 2, -3, None)
    return {
        "2/-5,-10/-1": (dna(2, -5, b"N"), -10, -1, b"ACGT", True),
        "5/-9,-2/-2": (dna(5, -9, b"N"), -2, -2, b"ACGT", True),
        "3/-3,-4/0": (dna(3, -3, b"N"), -4, 0, b"ACGT", True),
        "9/-20,-20/-5": (dna(9, -20, b"N"), -20, -5, b"ACGT", True),
        "1/-1,-2/-1": (dna(1, -1, b"N"), -2, -1, b"ACGT", True),
        "asym,-8/-1": (asym, -8, -1, b"ACGT", True),
        "acg,-6/-1": (acg, -6, -1, b"ACG", True),
        "2/-5,-1/-1 (refused)": (dna(2, -5, b"N"), -1, -1, b"ACGT", False),
    }


def _reference(alphabet: bytes, length: int, seed: int) -> bytes:
    from zoe_amd import synth

    if alphabet == b"ACGT":
        ref = bytearray(synth.reference_host(length))
    else:
        rng = np.random.default_rng(seed)
        ref = bytearray(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), length)].tobytes())
    for i in range(400 + 3, 460):  # a tandem repeat and homopolymer runs
        ref[i] = ref[i - 3]
    for at in range(900, length - 40, 97):
        ref[at:at + 6] = bytes([ref[at]]) * 6
    return bytes(ref)


def _edited_reads(rng, ref: bytes, n: int, L: int, alphabet: bytes) -> np.ndarray:
    """copies with 0-4 substitutions, single indels (inside homopolymer runs for a third of them), indel pairs a few bases apart"""
    r = np.frombuffer(ref, dtype=np.uint8)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    out = np.empty((n, L), dtype=np.uint8)
    runs = np.nonzero((r[1:-1] == r[:-2]) & (r[1:-1] == r[2:]))[0] + 1
    for i in range(n):
        kind = i % 5
        p = int(rng.integers(10, len(r) - L - 20))
        q = list(r[p:p + L + 16])
        if kind in (1, 2):  # one indel, in a run of equal bases for kind 2
            at = int(rng.integers(8, L - 8))
            if kind == 2 and len(runs):
                near = runs[(runs > p + 8) & (runs < p + L - 8)]
                if len(near):
                    at = int(near[rng.integers(0, len(near))]) - p
            g = 1 if rng.integers(0, 4) else int(rng.integers(2, 5))
            q = q[:at] + q[at + g:] if rng.integers(0, 2) else q[:at] + list(alpha[rng.integers(0, len(alpha), g)]) + q[at:]
        elif kind == 3:  # an indel pair a few bases apart
            a1 = int(rng.integers(8, L - 20))
            a2 = a1 + int(rng.integers(2, 10))
            g1, g2 = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            q = q[:a1] + q[a1 + g1:a2] + list(alpha[rng.integers(0, len(alpha), g2)]) + q[a2:]
        q = np.array(q[:L], dtype=np.uint8)
        for k in rng.choice(L, int(rng.integers(0, 5 if kind in (0, 4) else 2)), replace=False):
            q[k] = alpha[(int(np.where(alpha == q[k])[0][0]) + int(rng.integers(1, len(alpha)))) % len(alpha)] if q[k] in alpha else q[k]
        out[i] = q
    return out


def _read_set(rng, ref: bytes, alphabet: bytes, L: int, n: int) -> np.ndarray:
    from test_gpu_bounds import diverged_reads
    from test_gpu_shared import _tie_rich_reads
    from zoe_amd import synth

    if alphabet != b"ACGT":
        return _edited_reads(rng, ref, n, L, alphabet)
    parts = [synth.reads_host(ref, int(rng.integers(0, 1000)), n // 2, L), _edited_reads(rng, ref, n // 4, L, alphabet),
             _tie_rich_reads(rng, ref, n // 8, L), diverged_reads(ref, n - n // 2 - n // 4 - n // 8, L, 30, int(rng.integers(0, 1000)))]
    return np.concatenate(parts)


def _run(za, role, prof, rb, ref, src_is_query, records=None):
    import torch

    ctx = za.SwContext.get(0)
    ctx.debug_cert_records(records)
    try:
        if role == "read":
            a = prof.sw_align(za.SeqSrc.Query(ref) if src_is_query else za.SeqSrc.Reference(ref))
        else:
            a = prof.sw_align(za.SeqBatchSrc.Query(rb) if src_is_query else za.SeqBatchSrc.Reference(rb))
        torch.cuda.synchronize()
    finally:
        ctx.debug_cert_records(None)
    return a


def _check(za, model, oracle, role, scheme, T, N, L, n):
    import torch

    from test_gpu_shared import okey, osc
    from zoe_amd import _lib

    matrix, go, ge, alphabet, engages = _matrices(za)[scheme]
    rng = np.random.default_rng(stable_seed("cert", role, scheme, T, N, L))
    ref = _reference(alphabet, 2000 if role == "read" else 1800, stable_seed("cert-ref", scheme))
    reads = _read_set(rng, ref, alphabet, L, n)
    ctx = za.SwContext.get(0)
    m = matrix.to_biased_matrix() if T.startswith("u") else matrix
    rb = za.ReadBatch.from_fixed(torch.from_numpy(np.ascontiguousarray(reads).reshape(-1)).cuda(), L)
    if role == "read":
        prof = za.StripedProfileBatch(rb, m, go, ge, T, N)
    else:
        prof = za.SharedStripedProfile(ref, m, go, ge, T, N)
    rec_t = torch.full((n, 4), UNSET, dtype=torch.int32, device="cuda")
    got = _run(za, role, prof, rb, ref, False, rec_t)
    gotq = _run(za, role, prof, rb, ref, True)
    ctx.debug_set(_lib.DEBUG_ALIGN_NO_CERTIFICATE)
    try:
        want = _run(za, role, prof, rb, ref, False)
        wantq = _run(za, role, prof, rb, ref, True)
    finally:
        ctx.debug_set(0)
    # 1. the certificate changes nothing
    for a, b in ((got, want), (gotq, wantq)):
        assert np.array_equal(a.status, b.status)
        assert (a.tier is None) == (b.tier is None) and (a.tier is None or np.array_equal(a.tier, b.tier))
        assert np.array_equal(a.records, b.records)
        assert np.array_equal(a.inc, b.inc) and np.array_equal(a.op, b.op)
    rec = rec_t.cpu().numpy()
    written = rec[:, 0] != UNSET
    some = got.status == za.alignment.SOME
    counts = {name: int((rec[written, 0] == v).sum()) for v, name in enumerate(
        ["not_unique", "gapless", "one_gap", "diag_sum", "potential", "two_runs", "placement", "deferred"])}
    counts["sweep_launch"] = int((rec[written, 3] == 1).sum())
    print(f"\n[{role} {scheme} {T}x{N} L={L}] reads {n}, records {int(written.sum())}: {counts}")
    assert counts["deferred"] == 0, "a deferred read was not decided by the sweep launch"
    # 2. the kernel's records equal the host verdicts (on the reads whose first-pass values the records of the call carry)
    w = np.ascontiguousarray(matrix.signed_weights().astype(np.int32))
    S = w.shape[0]
    idx = matrix.mapping.index_map
    ref_idx = np.ascontiguousarray(idx[np.frombuffer(ref, dtype=np.uint8)])
    sel = np.nonzero(written & some)[0]
    r = got.records[sel]
    m_n = len(sel)
    sub_reads = np.ascontiguousarray(idx[reads[sel]]).reshape(-1)
    sub_off = np.arange(m_n + 1, dtype=np.uint64) * L
    cols = [np.ascontiguousarray(r[c].astype(np.uint32)) for c in ("score", "ref_start", "ref_end", "query_start", "query_end")]
    uniq = np.ascontiguousarray((rec[sel, 0] != NOT_UNIQUE).astype(np.uint8))
    host = np.zeros((m_n, 4), dtype=np.int32)
    shared = 1 if role == "shared" else 0
    rc = model.zsw_model_cert_verdicts(w.ctypes.data, S, -go, -ge, ref_idx.ctypes.data, len(ref_idx), sub_reads.ctypes.data, sub_off.ctypes.data, m_n,
                                       shared, *[c.ctypes.data for c in cols], uniq.ctypes.data, host.ctypes.data)
    assert rc == 0
    bad = np.nonzero((host != rec[sel]).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} reads: kernel {rec[sel][bad[:5]].tolist()} vs host {host[bad[:5]].tolist()} (reads {sel[bad[:5]].tolist()})"
    # 3. a sample of reads flagged unique: unique maxima at the reported corners; certified ones have exactly the certified alignments
    flagged = sel[rec[sel, 0] != NOT_UNIQUE]
    sample = flagged[np.linspace(0, len(flagged) - 1, min(len(flagged), 100)).astype(int)] if len(flagged) else flagged
    if engages:
        assert len(sample) >= 100
    want_n = np.ascontiguousarray(np.array([1 if rec[i, 0] == GAPLESS else rec[i, 2] if rec[i, 0] == ONE_GAP else 0 for i in sample], dtype=np.int32))
    sreads = np.ascontiguousarray(idx[reads[sample]]).reshape(-1)
    soff = np.arange(len(sample) + 1, dtype=np.uint64) * L
    cor = np.zeros((len(sample), 6), dtype=np.int32)
    if len(sample):
        assert model.zsw_model_cert_corners(w.ctypes.data, S, -go, -ge, ref_idx.ctypes.data, len(ref_idx), sreads.ctypes.data, soff.ctypes.data, len(sample),
                                            shared, want_n.ctypes.data, cor.ctypes.data) == 0
    for k, i in enumerate(sample):
        rr = got.records[i]
        assert cor[k, 0] != -1, f"read {i}: the optimal alignments between the corners are not the certified {want_n[k]}"
        assert cor[k, 0] == 1, f"read {i}: flagged unique, but a maximum sits in several cells"
        assert tuple(cor[k, 1:]) == (rr["score"], rr["ref_start"], rr["ref_end"], rr["query_start"], rr["query_end"]), i
    # 4. the oracle's literal sw_simd_align on a sample
    sc = osc(oracle, matrix, go, ge)
    for i in range(0, n, max(1, n // 40)):
        if role == "read":
            assert got.key(i) == okey(oracle.align(T, N, sc, bytes(reads[i]), ref)), i
        else:
            assert gotq.key(i) == okey(oracle.align(T, N, sc, ref, bytes(reads[i]), other_is_query=True)), i
    # 5. not vacuous
    if not engages:
        # (the read-as-profile role does not enter certificate mode; the shared role's seeded passes settle no read)
        assert counts["gapless"] == 0 and counts["one_gap"] == 0 and counts["not_unique"] == int(written.sum()), counts
        return counts
    assert counts["gapless"] >= 0.05 * n, counts
    if ge == 0:
        assert counts["one_gap"] == 0, counts
    elif L >= 100:
        assert counts["one_gap"] >= 0.01 * n, counts
    return counts


SCHEMES = ["2/-5,-10/-1", "5/-9,-2/-2", "3/-3,-4/0", "9/-20,-20/-5", "1/-1,-2/-1", "asym,-8/-1", "acg,-6/-1", "2/-5,-1/-1 (refused)"]


@pytest.mark.parametrize("role", ["read", "shared"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_certificate_verdicts_equal_the_header_on_the_host_i16(za, model, oracle, role, scheme):
    """<i16, 16>, 150 bp, 10,240 reads per scheme and role."""
    _check(za, model, oracle, role, scheme, "i16", 16, 150, 10240)


@pytest.mark.parametrize("role", ["read", "shared"])
@pytest.mark.parametrize("T,N", [("u16", 16), ("i32", 8)])
@pytest.mark.parametrize("scheme", ["2/-5,-10/-1", "3/-3,-4/0", "asym,-8/-1"])
def test_certificate_verdicts_equal_the_header_on_the_host_wide(za, model, oracle, role, T, N, scheme):
    """<u16, 16> (biased matrix) and <i32, 8> on three schemes, 10,240 reads each."""
    _check(za, model, oracle, role, scheme, T, N, 150, 10240)


@pytest.mark.parametrize("role", ["read", "shared"])
@pytest.mark.parametrize("T,scheme,L", [("i8", "2/-5,-10/-1", 64), ("u8", "5/-9,-2/-2", 50)])
def test_certificate_verdicts_equal_the_header_on_the_host_8bit(za, model, oracle, role, T, scheme, L):
    """<i8 / u8, 32> on short reads whose scores straddle the 8-bit limit (a copy scores 128 against 127 in i8, 250 against 246 in
    u8 with the bias of 9): the certificate's status comes from the seeded ranges pass, the literal path's from its own first pass."""
    _check(za, model, oracle, role, scheme, T, 32, L, 10240)
