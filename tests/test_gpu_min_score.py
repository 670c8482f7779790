"""ZSW_OPTION_MIN_SCORE (include/zoe_sw.h): with a minimum score T the covered entry points report a read that is UNMAPPED, or SOME
with a score below min(T, the overflow threshold of the call's last width), as ZSW_STATUS_BELOW_MIN_SCORE with every other field
0 — settled by the seeded pass's upper bounds where those suffice (the whole-read bound in the seed kernel, the bounds of a band
walk), by the exact score otherwise — and every other read exactly as with T = 0, whichever route settled it.

A wrong comparison here leaves reads unwritten rather than wrong, so every call goes through the C ABI with caller-owned arrays
filled with 0xA5 and EVERY read is compared. The reads are those of tests/test_gpu_seed_thresholds.py (300-base random reference,
150-base reads: junk without a shared 8-mer, clean copies, arrivals with a twelve-base deletion, diverged reads of abi_helpers),
the oracle scores each distinct read once, and the expectation is the contract applied to the oracle's result. The bounds come
from the host model (tests/models/min_score.cpp as a library), never from a constant: U_junk, the whole-read bound of a junk read,
is what that model computes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import abi_helpers as ah
import test_gpu_seed_thresholds as st
from conftest import ROOT

pytestmark = pytest.mark.gpu

L, REF_LEN, K = st.L, st.REF_LEN, st.K
BELOW = 4
OPTION_MIN_SCORE = 2
T_MAX = 2 ** 31 - 1
THR_I8, THR_I16, THR_I32 = 255, 65535, 2 ** 32 - 1
SEED_DN, SEED_DM, SEED_TOL, SEED_MIN_LEN = 4, 4, 8, 24  # zsw_score_seed.hpp
COVERED = ["zsw_score_batch", "zsw_score_batch_from", "zsw_score_ends_batch", "zsw_score_ranges_batch", "zsw_score_ranges_batch_from",
           "zsw_align_3pass_batch", "zsw_align_3pass_batch_from"]


class World:
    pass


@pytest.fixture(scope="module")
def model():
    d = tempfile.mkdtemp(prefix="zsw_min_score_model_")
    so = os.path.join(d, "libmin_score_model.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DZSW_MIN_SCORE_LIB", "-Wno-unknown-pragmas", "-o", so,
                    os.path.join(ROOT, "tests", "models", "min_score.cpp")], check=True)
    lib = C.CDLL(so)
    lib.zsw_model_min_whole.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    lib.zsw_model_band.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 11 + [C.c_void_p]
    lib.zsw_model_band_upper.argtypes = [C.c_uint32, C.c_int, C.c_int]
    lib.zsw_model_below_min.argtypes = [C.c_longlong, C.c_longlong]
    return lib


@pytest.fixture(scope="module")
def world(oracle, model):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib

    w = World()
    w._lib, w.lib, w.oracle, w.model = _lib, _lib.load(), oracle, model
    ref = ah.ACGT[np.random.default_rng(300).integers(0, 4, REF_LEN)]
    w.ref = ref.tobytes()
    present = np.zeros(4 ** K, dtype=bool)
    present[st._kmer_codes(ref[None, :])[0]] = True
    cand = ah.ACGT[np.random.default_rng(12345).integers(0, 4, (6000, L))]
    junk = cand[~present[st._kmer_codes(cand)].any(axis=1)]
    assert len(junk) >= 2048, len(junk)
    clean = np.stack([ref[s:s + L] for s in range(REF_LEN - L + 1)])
    arrivals = np.stack([np.concatenate([ref[s:s + st.GAP_AT], ref[s + st.GAP_AT + st.GAP:s + L + st.GAP]]) for s in range(REF_LEN - L - st.GAP + 1)])
    rng = np.random.default_rng(7)
    mutated = np.stack([np.frombuffer(ah._one_read(rng, ref, L, "diverged", i)[0], dtype=np.uint8) for i in range(2000)])
    # a copy with six substitutions, twenty bases apart: 300 - 6 * 7 = 258, inside [255, 260)
    near = ref[40:40 + L].copy()
    for c in range(20, 140, 20):
        near[c] = ah.ACGT[(int(np.where(ah.ACGT == near[c])[0][0]) + 1) % 4]
    w.pool = np.ascontiguousarray(np.concatenate([junk, clean, arrivals, mutated, near[None, :]]))
    w.junk0, w.n_junk = 0, len(junk)
    w.clean0, w.n_clean = len(junk), len(clean)
    w.arr0, w.n_arr = w.clean0 + len(clean), len(arrivals)
    w.mut0, w.n_mut = w.arr0 + len(arrivals), len(mutated)
    w.near = w.mut0 + len(mutated)
    w.dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    w.sc = oracle.Scoring(w.dna.signed_weights(), w.dna.mapping.index_map, -10, -1)
    w.want = oracle.batch_score_w256(8, w.sc, w.pool, w.ref, fixed_len=L, threads=16)
    # (the cascade ends at i32: every read has a status SOME or UNMAPPED and its true score)
    assert np.isin(w.want[1], (ah.S_, ah.U_)).all()
    w.true = np.where(w.want[1] == ah.S_, w.want[0], 0).astype(np.int64)
    assert 255 <= w.true[w.near] < 260, w.true[w.near]
    assert (w.true[w.clean0:w.clean0 + w.n_clean] == 300).all() and w.true[:w.n_junk].max() < 60
    w.ends = {}
    w.h = ah.new_context(_lib, w.lib, w.dna, -10, -1, w.ref, pseq=w.ref)
    # the whole-read bound of every pool read, as the seed kernel derives it
    w.whole = whole_bounds(w, w.pool.reshape(-1), np.arange(len(w.pool) + 1, dtype=np.int64) * L)
    u = np.unique(w.whole[:w.n_junk])
    assert len(u) == 1, u  # none of a junk read's k-mers occurs: the same bound for all of them
    w.u_junk = int(u[0])
    assert w.true[:w.n_junk].max() < w.u_junk < 250
    yield w
    set_min(w, 0)
    w.lib.zsw_debug_set(w.h, 0)
    w.lib.zsw_destroy(w.h)


def whole_bounds(w, flat, off):
    idx = np.ascontiguousarray(w.dna.mapping.index_map[np.ascontiguousarray(flat, dtype=np.uint8)]) if len(flat) else np.zeros(1, dtype=np.uint8)
    ref_idx = np.ascontiguousarray(w.dna.mapping.index_map[np.frombuffer(w.ref, dtype=np.uint8)])
    wt = np.ascontiguousarray(w.dna.signed_weights().astype(np.int32))
    off = np.ascontiguousarray(off, dtype=np.int64)
    out = np.zeros(len(off) - 1, dtype=np.int32)
    rc = w.model.zsw_model_min_whole(wt.ctypes.data, wt.shape[0], 10, 1, ref_idx.ctypes.data, len(ref_idx), idx.ctypes.data, off.ctypes.data, len(off) - 1, K, SEED_TOL,
                                     SEED_MIN_LEN, out.ctypes.data)
    assert rc == 0
    return out.astype(np.int64)


def set_min(w, t, rc=0):
    assert w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(t)) == rc, (t, w.lib.zsw_last_error_string(w.h).decode())


def counts(w):
    c = (C.c_uint64 * 4)()
    assert w.lib.zsw_min_score_counts(w.h, c) == 0
    return [int(x) for x in c]


def thr_of(entry, T="i16"):
    return THR_I32 if ah.ENTRY[entry].cascade else {"i8": THR_I8, "i16": THR_I16}[T]


def run(w, entry, rs, pres, t, T=None, records=False, flags=0):
    """One call with minimum score t on sentinel-filled arrays -> (result arrays, zsw_prune_rescored, the four counters, records)"""
    import torch

    set_min(w, t)
    assert w.lib.zsw_debug_set(w.h, flags) == 0
    p = ah.Presented(w._lib, rs, pres, lib=w.lib, h=w.h, index_map=w.dna.mapping.index_map)
    rec = None
    if records:
        rec = torch.zeros(8 * rs.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert w.lib.zsw_debug_band_records(w.h, rec.data_ptr()) == 0
    try:
        c = ah.Call(w._lib, w.lib, w.h, ah.ENTRY[entry], p, T=T).run()
        assert c.rc == 0, w.lib.zsw_last_error_string(w.h).decode()
        torch.cuda.synchronize()
        back, cnt = st.rescored(w), counts(w)
    finally:
        if records:
            assert w.lib.zsw_debug_band_records(w.h, None) == 0
        assert w.lib.zsw_debug_set(w.h, 0) == 0
        set_min(w, 0)
    res = {k: a.data() for k, a in c.out.items()}
    assert all(a.guards_intact() for a in c.out.values()), (entry, "guard entries were written")
    unscored = int((res["status"] == ah.FILL).sum())
    assert unscored == 0, (entry, t, f"{unscored} of {rs.n} reads were never written: their statuses are still the caller's fill")
    return res, back, cnt, (rec.cpu().numpy().reshape(rs.n, 8) if records else None)


def cigars(res):
    """per read: the CIGAR of its record, '' without ciglets"""
    out = []
    for r in res["aln"]:
        o, n = int(r["ciglet_offset"]), int(r["n_ciglets"])
        out.append("".join(f"{int(res['inc'][o + k])}{chr(int(res['op'][o + k]))}" for k in range(n)))
    return out


def below_mask(w, idx, t, thr):
    true = w.true[idx]
    return (true == 0) | (true < min(t, thr)) if t > 0 else np.zeros(len(idx), dtype=bool)


def check_contract(w, entry, res, base, idx, t, thr, what):
    """`res` (minimum t) against the contract: the reads below min(t, thr) by the ORACLE's score are BELOW with every field 0, the
    others are bit for bit `base`, the same call with t = 0 (whose scores, statuses and tiers are the oracle's: checked by the
    caller). Alignment records are compared field by field but for ciglet_offset, and CIGAR by CIGAR."""
    below = below_mask(w, idx, t, thr)
    assert not (below & (base["status"] == ah.O_)).any()
    want_status = np.where(below, BELOW, base["status"]).astype(np.uint8)
    bad = np.nonzero(res["status"] != want_status)[0]
    assert len(bad) == 0, (what, "status", f"{len(bad)} reads differ, first {bad[:5]}: got {res['status'][bad[:5]]}, want {want_status[bad[:5]]}, true {w.true[idx][bad[:5]]}")
    for k in res:
        if k in ("status", "inc", "op"):
            continue
        if k == "aln":
            for f in ah.ALN_DTYPE.names:
                if f == "ciglet_offset":
                    continue
                want = np.where(below, 0, base["aln"][f])
                bad = np.nonzero(res["aln"][f] != want)[0]
                assert len(bad) == 0, (what, f"aln.{f}", f"{len(bad)} reads differ, first {bad[:5]}: got {res['aln'][f][bad[:5]]}, want {want[bad[:5]]}")
            assert (res["aln"]["ciglet_offset"][below] == 0).all(), (what, "a read below the minimum has a ciglet offset")
            want_cig = [("" if b else c) for b, c in zip(below, cigars(base))]
            assert cigars(res) == want_cig, (what, "CIGARs differ")
            assert len(res["inc"]) == int(res["aln"]["n_ciglets"].sum()) == int(np.where(below, 0, base["aln"]["n_ciglets"]).sum()), (what, "ciglet total")
            continue
        want = np.where(below, 0, base[k]).astype(base[k].dtype)
        bad = np.nonzero(res[k] != want)[0]
        assert len(bad) == 0, (what, k, f"{len(bad)} reads differ, first {bad[:5]}: got {res[k][bad[:5]]}, want {want[bad[:5]]}")
    return below


def check_base(w, entry, base, idx, thr):
    """the t = 0 call against the oracle: score and status of every read (tier for the _from calls)"""
    true = w.true[idx]
    st_want = np.where(true >= thr, ah.O_, np.where(true == 0, ah.U_, ah.S_)).astype(np.uint8)
    assert np.array_equal(base["status"], st_want), entry
    score = base["aln"]["score"] if "aln" in base else base["score"]
    assert np.array_equal(score.astype(np.int64), np.where(st_want == ah.S_, true, 0)), entry
    if "tier" in base:
        assert np.array_equal(base["tier"], w.want[2][idx]), entry


def mixed_idx(w):
    idx = np.concatenate([st.junk_idx(w, 1024), st.even_idx(w.clean0, w.n_clean, 1024), st.even_idx(w.arr0, w.n_arr, 510), w.mut0 + np.arange(1536) % w.n_mut,
                          np.full(2, w.near)])
    return st.shuffled(idx)


# ---- 1. the contract over a grid of T ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", COVERED)
def test_contract_over_a_grid_of_minimum_scores(world, entry):
    """4,096 reads (junk, copies, arrivals, diverged, and a read of score 258) through one covered entry point, direct calls at
    I16 and _from calls at 8 / 256, for T in {0, 1, U_junk, U_junk + 1, 250, 300, 301, 2^31 - 1}: score, status, tier, ends, ranges,
    records and CIGARs of every read against the contract on the oracle's score and against the T = 0 call. T = 0 changes nothing
    and counts nothing; at 301 no read is SOME; at 2^31 - 1 neither, and none is OVERFLOWED."""
    w = world
    idx = mixed_idx(w)
    rs = st.fixed_set(w, idx, "grid")
    thr = thr_of(entry)
    base, back0, cnt0, _ = run(w, entry, rs, "device-fixed", 0)
    check_base(w, entry, base, idx, thr)
    assert cnt0 == [0, 0, 0, 0]
    for t in (1, w.u_junk, w.u_junk + 1, 250, 300, 301, T_MAX):
        res, back, cnt, _ = run(w, entry, rs, "device-fixed", t)
        below = check_contract(w, entry, res, base, idx, t, thr, (entry, t))
        print(f"{entry} T {t}: below {int(below.sum())}, counts {cnt}, zsw_prune_rescored {back} (T = 0: {back0})")
        assert cnt[3] == cnt[0] + cnt[1] + cnt[2] == int(below.sum())
        assert back <= back0 and back + cnt[0] + cnt[1] <= rs.n
        if t > 300:
            assert (res["status"] == BELOW).all()
        if t <= w.u_junk:
            assert cnt[0] == 0  # no read of this batch has a whole-read bound below U_junk
        else:
            assert cnt[0] >= 1024


# ---- 2. the threshold itself --------------------------------------------------------------------------------------------------------
def test_whole_read_bound_settles_junk_exactly_above_its_bound(world):
    """2,048 junk reads and 2,048 copies. The junk reads' whole-read bound is U_junk: with T = 0 and T = U_junk the bound is not
    below T, every junk read is handed back and scored over all its cells (zsw_prune_rescored = 2,048; at T = U_junk the exact
    score then puts it below); with T = U_junk + 1 the seed kernel settles all of them: nothing is handed back, and the results
    are those of T = U_junk."""
    w = world
    n_junk = 2048
    idx = st.shuffled(np.concatenate([st.junk_idx(w, n_junk), st.even_idx(w.clean0, w.n_clean, 2048)]))
    rs = st.fixed_set(w, idx, "threshold")
    base, back0, cnt0, _ = run(w, "zsw_score_batch_from", rs, "device-fixed", 0)
    check_base(w, "zsw_score_batch_from", base, idx, THR_I32)
    assert back0 == n_junk and cnt0 == [0, 0, 0, 0]
    at, back_at, cnt_at, _ = run(w, "zsw_score_batch_from", rs, "device-fixed", w.u_junk)
    check_contract(w, "zsw_score_batch_from", at, base, idx, w.u_junk, THR_I32, "T = U_junk")
    assert back_at == n_junk and cnt_at == [0, 0, n_junk, n_junk], (back_at, cnt_at)
    above, back_above, cnt_above, _ = run(w, "zsw_score_batch_from", rs, "device-fixed", w.u_junk + 1)
    check_contract(w, "zsw_score_batch_from", above, base, idx, w.u_junk + 1, THR_I32, "T = U_junk + 1")
    assert back_above == 0 and cnt_above == [n_junk, 0, 0, n_junk], (back_above, cnt_above)
    ah.assert_same(above, at, "T = U_junk + 1 against T = U_junk")


# ---- 3. the band route --------------------------------------------------------------------------------------------------------------
def model_walk(w, read, g, tag=-1):
    """zsw_model_band for one read with the geometry of its debug record -> (maximum2, oa, ob)"""
    im = w.dna.mapping.index_map
    wt = np.ascontiguousarray(w.dna.signed_weights().astype(np.int32))
    ref_idx = np.ascontiguousarray(im[np.frombuffer(w.ref, dtype=np.uint8)])
    q = np.ascontiguousarray(im[read])
    out = np.zeros(8, dtype=np.int32)
    n_strips, wu, wd = int(g[5] & 0xff), int((g[5] >> 8) & 0xfff), int((g[5] >> 20) & 0xfff)
    rc = w.model.zsw_model_band(wt.ctypes.data, wt.shape[0], 10, 1, ref_idx.ctypes.data, len(ref_idx), q.ctypes.data, len(q), K, SEED_DN, SEED_DM, SEED_TOL,
                                int(g[7]) >> 8, n_strips, wu, wd, int(g[3]), int(g[4]), tag, out.ctypes.data)
    assert rc == 0 and out[0] == 1
    return int(out[2]), max(int(out[3]), 0), max(int(out[4]), 0)


def band_upper(w, rec):
    return np.array([w.model.zsw_model_band_upper(int(r[0]) & 0xffffffff, int(r[1]), int(r[2])) for r in rec], dtype=np.int64)


def test_band_bounds_settle_diverged_reads_in_either_tier(world):
    """4,096 diverged reads (3 - 12 % substitutions, half of them with an indel) and 1,024 copies through both band tiers (the
    any-size switch gives a small batch the two tiers of a large one). A first run with T = 0 and the band's debug records picks
    T: the smallest of 200, 210, ..., 280 for which at least 50 reads are walked, not accepted, and have a band bound —
    seed_band_upper of the walk's maximum, oa and ob — below T; the host model recomputes those walks and must agree. With that T:
    a walked, unaccepted read is settled by the band exactly when seed_band_upper of its record is below T; counts[1] is their
    number; a read the first tier settles keeps the first tier's record (the second tier never saw it); results are the contract's."""
    w = world
    flags = w._lib.DEBUG_SCORE_PRUNE_ANY_SIZE
    idx = st.shuffled(np.concatenate([w.mut0 + np.arange(4096) % w.n_mut, st.even_idx(w.clean0, w.n_clean, 1024)]))
    rs = st.fixed_set(w, idx, "band")
    base, back0, _, rec0 = run(w, "zsw_score_batch_from", rs, "device-fixed", 0, records=True, flags=flags)
    check_base(w, "zsw_score_batch_from", base, idx, THR_I32)
    walked0, refused0 = rec0[:, 5] != 0, (rec0[:, 5] != 0) & ((rec0[:, 7] & 1) == 0)
    up0 = band_upper(w, rec0)
    assert (up0[walked0] >= w.true[idx][walked0]).all(), "a band bound below the read's score"
    T = next((t for t in range(200, 290, 10) if int((refused0 & (up0 < t)).sum()) >= 50), None)
    assert T is not None, "no T up to 280 leaves 50 refused walks with a bound below it"
    pre = np.nonzero(refused0 & (up0 < T))[0]
    for i in pre[:200]:  # the model on the same walks: the kernel's values are the model's, so the precondition is the model's too
        assert model_walk(w, w.pool[idx[i]], rec0[i]) == (int(rec0[i, 0]), max(int(rec0[i, 1]), 0), max(int(rec0[i, 2]), 0)), i
    assert w.model.zsw_model_below_min(T - 1, T) == 1 and w.model.zsw_model_below_min(T, T) == 0
    res, back, cnt, rec = run(w, "zsw_score_batch_from", rs, "device-fixed", T, records=True, flags=flags)
    below = check_contract(w, "zsw_score_batch_from", res, base, idx, T, THR_I32, ("band", T))
    walked, refused = rec[:, 5] != 0, (rec[:, 5] != 0) & ((rec[:, 7] & 1) == 0)
    up = band_upper(w, rec)
    by_band = refused & (up < T)
    by_seed = w.whole[idx] < T
    print(f"T {T}: precondition {len(pre)}; below {int(below.sum())}, by the band {int(by_band.sum())} (first tier {int((by_band & ((rec[:, 7] >> 8) == 1)).sum())}), "
          f"by the seed kernel {int(by_seed.sum())}; counts {cnt}; zsw_prune_rescored {back} (T = 0: {back0})")
    assert int(by_band.sum()) >= 50
    assert not (walked & by_seed).any(), "a read the seed kernel settled was walked"
    assert (res["status"][by_band] == BELOW).all()
    assert cnt[0] == int(by_seed.sum()) and cnt[1] == int(by_band.sum()) and cnt[3] == int(below.sum())
    # a refused walk whose bound is not below T went on: to the second tier, or to the full pass — and none of those counts as settled
    first = (rec[:, 7] >> 8) == 1
    moved = by_band & first & ((rec0[:, 7] >> 8) == 48)
    assert int(moved.sum()) >= 1, "no read that reached the second tier at T = 0 was settled by the first tier"
    # handed back: every read that was neither accepted nor settled (which reads the second tier accepts depends on their lane
    # partners, and those change when the first tier settles reads: this run's own records count, not the T = 0 run's)
    assert back == rs.n - int((rec[:, 7] & 1).sum()) - int(by_band.sum()) - int(by_seed.sum())
    assert back < back0


# ---- 4. overflow interplay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruning", [1, 0])
def test_direct_i8_call_keeps_overflowed_reads_overflowed(world, pruning):
    """zsw_score_batch at I8 (threshold 255) with T = 260: min(T, thr) = 255. Copies (score 300) and the read of score 258, which
    lies in [thr, T), stay OVERFLOWED; junk reads are BELOW — with the seeded pass and with ZSW_OPTION_EXACT_PRUNING 0."""
    w = world
    idx = st.shuffled(np.concatenate([st.junk_idx(w, 1024), st.even_idx(w.clean0, w.n_clean, 1024), np.full(64, w.near), w.mut0 + np.arange(1984) % w.n_mut]))
    rs = st.fixed_set(w, idx, "i8")
    assert w.lib.zsw_set_option(w.h, 1, C.c_int64(pruning)) == 0
    try:
        base, _, _, _ = run(w, "zsw_score_batch", rs, "device-fixed", 0, T="i8")
        check_base(w, "zsw_score_batch", base, idx, THR_I8)
        res, back, cnt, _ = run(w, "zsw_score_batch", rs, "device-fixed", 260, T="i8")
    finally:
        assert w.lib.zsw_set_option(w.h, 1, C.c_int64(1)) == 0
    check_contract(w, "zsw_score_batch", res, base, idx, 260, THR_I8, ("i8", pruning))
    true = w.true[idx]
    assert (res["status"][true >= 255] == ah.O_).all() and (res["status"][idx == w.near] == ah.O_).all()
    assert (res["status"][idx < w.n_junk] == BELOW).all()
    assert (cnt[0] >= 1024) if pruning else (cnt[:2] == [0, 0] and back == 0)


# ---- 5. a ragged batch ---------------------------------------------------------------------------------------------------------------
def test_ragged_batch_empty_and_short_reads(world):
    """Reads of 0 - 23 bases (too short to be swept: bounded by the potential of their columns, 2 per base) beside 150-base junk
    and copies, T = 30. Length 0 stays EMPTY; 1 - 14 bases (potential below 30) are BELOW without a hand-back; 15 - 23 bases are
    scored exactly — a copy of 20 bases keeps its 40, a random one falls below by its score."""
    w = world
    T = 30
    rng = np.random.default_rng(5)
    ref = np.frombuffer(w.ref, dtype=np.uint8)
    reads = []
    for i in range(2560):
        n = i % 24
        s = int(rng.integers(0, REF_LEN - 24))
        reads.append((ref[s:s + n] if i % 3 else ah.ACGT[rng.integers(0, 4, n)]).tobytes())
    long_idx = np.concatenate([st.junk_idx(w, 1024), st.even_idx(w.clean0, w.n_clean, 1024)])
    reads += [w.pool[i].tobytes() for i in long_idx]
    order = np.random.default_rng(6).permutation(len(reads))
    reads = [reads[i] for i in order]
    n = len(reads)
    lens = np.array([len(r) for r in reads])
    rs = ah.ReadSet("ragged", w.ref, reads, 0, np.zeros(n, dtype=np.int64), np.full(n, -1))
    # (the oracle's profile constructor refuses an empty read, as the reference's does: EMPTY with score and tier 0 is the library's)
    filled = [r for r in reads if r]
    off_f = np.zeros(len(filled) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in filled], out=off_f[1:])
    s_f, st_f, t_f = w.oracle.batch_score_w256(8, w.sc, np.frombuffer(b"".join(filled), dtype=np.uint8), w.ref, offsets=off_f, threads=16)
    score, status, tier = np.zeros(n, dtype=np.uint32), np.full(n, ah.E_, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    score[lens > 0], status[lens > 0], tier[lens > 0] = s_f, st_f, t_f
    assert (lens == 0).sum() >= 100 and np.isin(st_f, (ah.S_, ah.U_)).all()
    true = np.where(status == ah.S_, score, 0).astype(np.int64)
    whole = whole_bounds(w, rs.bases, rs.offsets.astype(np.int64))
    short = (lens > 0) & (lens < SEED_MIN_LEN)
    assert (whole[short] == 2 * lens[short]).all()
    base, back0, _, _ = run(w, "zsw_score_batch_from", rs, "device-ragged", 0)
    assert np.array_equal(base["status"], status) and np.array_equal(base["score"], score) and np.array_equal(base["tier"], tier)
    res, back, cnt, _ = run(w, "zsw_score_batch_from", rs, "device-ragged", T)
    below = (status != ah.E_) & ((true == 0) | (true < T))
    assert np.array_equal(res["status"], np.where(below, BELOW, status).astype(np.uint8))
    for k, v in (("score", score), ("tier", tier)):
        assert np.array_equal(res[k], np.where(below, 0, v).astype(v.dtype)), k
    by_bound = (lens > 0) & (whole < T)
    assert by_bound.sum() == (short & (lens < 15)).sum() >= 1000 and (res["status"][by_bound] == BELOW).all()
    exact_short = short & (lens >= 15)
    assert (res["status"][exact_short] == ah.S_).sum() >= 300 and (res["status"][exact_short] == BELOW).sum() >= 100
    print(f"ragged, T {T}: counts {cnt}, zsw_prune_rescored {back} (T = 0: {back0})")
    assert cnt[0] == int(by_bound.sum()) and cnt[1] == 0 and cnt[3] == int(below.sum())
    assert back == back0 - int(by_bound.sum())  # (no read of 1 - 23 bases has an anchor: at T = 0 every one of them is handed back)


# ---- 6. route independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["zsw_score_batch_from", "zsw_score_ends_batch", "zsw_align_3pass_batch_from"])
def test_every_route_gives_the_default_routes_arrays(world, entry):
    """T = U_junk + 24 (junk by the whole-read bound, diverged reads by band bounds and exact scores) on the mixed batch: the
    default route against ZSW_OPTION_EXACT_PRUNING 0, the window kernel instead of the band, two tiers with the diagonal and with
    the strip first tier, a host batch, a PACKED4 host batch, and a batch of 512 reads, too small for the seeded pass."""
    w = world
    idx = mixed_idx(w)
    rs = st.fixed_set(w, idx, "routes")
    t = w.u_junk + 24
    thr = thr_of(entry)
    base, _, _, _ = run(w, entry, rs, "device-fixed", 0)
    want, _, cnt, _ = run(w, entry, rs, "device-fixed", t)
    check_contract(w, entry, want, base, idx, t, thr, (entry, "default"))
    assert cnt[0] >= 1024
    D = w._lib
    for name, pres, flags, pruning in (("no pruning", "device-fixed", 0, 0), ("window kernel", "device-fixed", D.DEBUG_SEED_NO_BAND, 1),
                                       ("two tiers", "device-fixed", D.DEBUG_SCORE_PRUNE_ANY_SIZE, 1),
                                       ("two tiers, strips first", "device-fixed", D.DEBUG_SCORE_PRUNE_ANY_SIZE | D.DEBUG_SEED_STRIP_FIRST_TIER, 1),
                                       ("host", "host-fixed", 0, 1), ("host, packed", "host-packed4", 0, 1)):
        assert w.lib.zsw_set_option(w.h, 1, C.c_int64(pruning)) == 0
        try:
            got, back, c, _ = run(w, entry, rs, pres, t, flags=flags)
        finally:
            assert w.lib.zsw_set_option(w.h, 1, C.c_int64(1)) == 0
        print(f"{entry}, {name}: counts {c}, zsw_prune_rescored {back}")
        check_contract(w, entry, got, base, idx, t, thr, (entry, name))
        assert c[3] == cnt[3]
        if not pruning:
            assert c[:2] == [0, 0]
    small = st.fixed_set(w, idx[:512], "small")
    base_s, _, _, _ = run(w, entry, small, "device-fixed", 0)
    got, back, c, _ = run(w, entry, small, "device-fixed", t)
    check_contract(w, entry, got, base_s, idx[:512], t, thr, (entry, "512 reads"))
    assert back == 0 and c[:2] == [0, 0] and c[2] == c[3]


# ---- 7. the entry points the option does not cover ----------------------------------------------------------------------------------
def test_uncovered_entry_points_refuse_and_invalid_values_are_rejected(world):
    """zsw_align_batch(_from), the shared-profile calls and the strand-aware calls: with T > 0 each returns ZSW_ERR_UNSUPPORTED
    naming the option and writes nothing; after T = 0 each returns what it returned before. -1 and 2^31 are not values."""
    import torch

    w = world
    idx = mixed_idx(w)[:1536]
    rs = st.fixed_set(w, idx, "uncovered")
    names = [e.name for e in ah.ENTRIES if e.shared or e.name in ("zsw_align_batch", "zsw_align_batch_from")]
    assert len(names) == 11
    before = {}
    for name in names:
        c = ah.Call(w._lib, w.lib, w.h, ah.ENTRY[name], ah.Presented(w._lib, rs, "device-fixed")).run()
        before[name] = c.collect()

    def strands(t):
        """zsw_score_strands_batch_from and zsw_align_3pass_strands_batch_from by hand -> (rc, arrays) each"""
        p = ah.Presented(w._lib, rs, "device-fixed")
        o = {k: ah.Out(rs.n, ah.DTYPES[k], True) for k in ("score", "status", "tier", "aln")}
        strand = ah.Out(rs.n, np.uint8, True)
        rc1 = w.lib.zsw_score_strands_batch_from(w.h, p.ref(), 8, 256, o["score"].ptr, o["status"].ptr, o["tier"].ptr, strand.ptr, None)
        torch.cuda.synchronize()
        first = {k: o[k].fetch().copy() for k in ("score", "status", "tier")}, strand.fetch().copy()
        o2 = {k: ah.Out(rs.n, ah.DTYPES[k], True) for k in ("status", "tier", "aln")}
        strand2, total = ah.Out(rs.n, np.uint8, True), C.c_uint64(0)
        inc, op = ah.Out(8 * rs.n, np.uint32, True), ah.Out(8 * rs.n, np.uint8, True)
        rc2 = w.lib.zsw_align_3pass_strands_batch_from(w.h, p.ref(), 8, 256, 0, o2["aln"].ptr, o2["status"].ptr, o2["tier"].ptr, strand2.ptr, inc.ptr, op.ptr,
                                                       8 * rs.n, C.byref(total), None)
        torch.cuda.synchronize()
        second = {k: o2[k].fetch().copy() for k in o2}, strand2.fetch().copy(), inc.fetch().copy(), op.fetch().copy(), int(total.value)
        return rc1, first, rc2, second, [*o.values(), strand, *o2.values(), strand2, inc, op]

    rc1, first0, rc2, second0, _ = strands(0)
    assert rc1 == 0 and rc2 == 0
    for bad in (-1, 2 ** 31, 2 ** 40):
        set_min(w, bad, rc=-1)
    for good in (T_MAX, 225):
        set_min(w, good)
    try:
        for name in names:
            e = ah.ENTRY[name]
            c = ah.Call(w._lib, w.lib, w.h, e, ah.Presented(w._lib, rs, "device-fixed"))
            rc = c.fn(*(c._args(None, None, 0) if e.kind == "align" else c._args()))
            torch.cuda.synchronize()
            msg = w.lib.zsw_last_error_string(w.h).decode()
            assert rc == -4 and "ZSW_OPTION_MIN_SCORE" in msg and name in msg, (name, rc, msg)
            assert all(a.untouched() for a in c.out.values()) and c.total.value == 0, name
        rc1, _, rc2, _, outs = strands(225)
        assert rc1 == -4 and rc2 == -4 and all(a.untouched() for a in outs)
        assert "ZSW_OPTION_MIN_SCORE" in w.lib.zsw_last_error_string(w.h).decode()
    finally:
        set_min(w, 0)
    for name in names:
        c = ah.Call(w._lib, w.lib, w.h, ah.ENTRY[name], ah.Presented(w._lib, rs, "device-fixed")).run()
        ah.assert_same(c.collect(), before[name], name)
    rc1, first1, rc2, second1, _ = strands(0)
    assert rc1 == 0 and rc2 == 0
    for a, b in zip(first0[0].values(), first1[0].values()):
        assert np.array_equal(a, b)
    assert np.array_equal(first0[1], first1[1]) and second0[4] == second1[4]
    for a, b in zip(second0[0].values(), second1[0].values()):
        assert np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(second0[1:4], second1[1:4]))
