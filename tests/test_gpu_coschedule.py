"""The full pass over the seed kernel's hand-backs inside the first band tier's launch (zsw_score_band.hip: seed_diag_handback_kernel;
the decision and the grid split: zsw_handback.hpp). A score-only call of two band tiers with reads of up to 152 bases scores
fail_list[0, n0) — what the seed kernel listed — in the first blocks of the first tier's grid, and the gated launches behind the
band tiers score fail_list[n0, count) only. A wrong split gives no wrong score: it leaves reads unscored or scores them twice. So
every call goes through the C ABI with caller-owned arrays filled with 0xA5, EVERY read is compared with the oracle, no status may
keep the fill, zsw_prune_rescored must equal the count the rules predict, and every case runs again under
ZSW_DEBUG_SEED_NO_COSCHEDULE (the launches as they were) and must give the same arrays.

The reads are those of tests/test_gpu_seed_thresholds.py, at several lengths: junk (no 8-mer of the 300-base reference: never
anchored, listed by the seed kernel — they are n0), clean copies (the first tier proves them) and arrivals (a twelve-base deletion:
outside the first tier's band; the second tier walks them or, by its bail-out rules, hands them back unwalked BEHIND n0).
ZSW_DEBUG_SCORE_PRUNE_ANY_SIZE gives two tiers at these sizes."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah
import test_gpu_seed_thresholds as st

pytestmark = pytest.mark.gpu

REF_LEN, K = st.REF_LEN, st.K
L_MAX = 153
LENGTHS = (24, 76, 77, 100, 150, 152, 153)
CFG = {24: (4, 19), 76: (4, 19), 77: (4, 22), 100: (4, 25), 150: (4, 38), 152: (4, 38), 153: (8, 22)}  # first fit of zsw_score_v2.hpp's list
CUT = st.CUTS[0]
OPTION_MIN_SCORE = 2
BELOW = 4


class World:
    pass


@pytest.fixture(scope="module")
def world(oracle):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib

    w = World()
    w._lib, w.lib, w.oracle = _lib, _lib.load(), oracle
    ref = ah.ACGT[np.random.default_rng(300).integers(0, 4, REF_LEN)]
    w.ref = ref.tobytes()
    present = np.zeros(4 ** K, dtype=bool)
    present[st._kmer_codes(ref[None, :])[0]] = True
    cand = ah.ACGT[np.random.default_rng(4321).integers(0, 4, (14000, L_MAX))]
    junk = cand[~present[st._kmer_codes(cand)].any(axis=1)]
    assert len(junk) >= 4097, len(junk)
    junk = junk[:4097]
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    w.sc = oracle.Scoring(dna.signed_weights(), dna.mapping.index_map, -10, -1)
    # per length: the pool (junk prefixes, clean copies; at 150 bases the arrivals too) and the oracle's result for each pool read
    w.pool, w.want, w.clean0, w.n_clean, w.arr0, w.n_arr = {}, {}, {}, {}, 0, 0
    for ln in LENGTHS:
        parts = [junk[:, :ln], np.stack([ref[s:s + ln] for s in range(REF_LEN - ln + 1)])]
        w.clean0[ln], w.n_clean[ln] = len(junk), len(parts[1])
        if ln == st.L:
            parts.append(np.stack([np.concatenate([ref[s:s + st.GAP_AT], ref[s + st.GAP_AT + st.GAP:s + ln + st.GAP]]) for s in range(REF_LEN - ln - st.GAP + 1)]))
            w.arr0, w.n_arr = w.clean0[ln] + w.n_clean[ln], len(parts[2])
        w.pool[ln] = np.ascontiguousarray(np.concatenate(parts))
        w.want[ln] = oracle.batch_score_w256(8, w.sc, w.pool[ln], w.ref, fixed_len=ln, threads=16)
        assert (w.want[ln][1][:len(junk)] == ah.S_).all()  # junk: a score, if a small one
    w.n_junk = len(junk)
    w.h = ah.new_context(_lib, w.lib, dna, -10, -1, w.ref)
    yield w
    w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(0))
    w.lib.zsw_debug_set(w.h, 0)
    w.lib.zsw_destroy(w.h)


def read_set(w, ln, idx, name):
    reads = w.pool[ln][idx]
    return ah.ReadSet(name, w.ref, reads, ln, np.zeros(len(idx), dtype=np.int64), np.full(len(idx), -1), _flat=reads.reshape(-1))


def both_ways(w, rs, pres, records=False):
    """the call co-scheduled (by default, where the decision holds) and with the launches as they were"""
    out = []
    for flags in (w._lib.DEBUG_SCORE_PRUNE_ANY_SIZE, w._lib.DEBUG_SCORE_PRUNE_ANY_SIZE | w._lib.DEBUG_SEED_NO_COSCHEDULE):
        assert w.lib.zsw_debug_set(w.h, flags) == 0
        try:
            out.append(st.call(w, "zsw_score_batch_from", rs, pres, records=records))
        finally:
            assert w.lib.zsw_debug_set(w.h, 0) == 0
    (res, back, log, rec7), (res_no, back_no, log_no, _) = out
    for k in res:
        assert np.array_equal(res[k], res_no[k]), (rs.name, k, "differs from the call under ZSW_DEBUG_SEED_NO_COSCHEDULE")
    assert back == back_no, (rs.name, back, back_no)
    return res, back, log, log_no, rec7


def check_logs(w, log, log_no, cfg, coscheduled, classes=1):
    """co-scheduled: two SEED_BAND records per class and one V2 (4, C, 0) record more than the launches as they were; otherwise the same log"""
    V2, BAND = w._lib.LAUNCH_V2, w._lib.LAUNCH_SEED_BAND
    assert len([r for r in log_no if r[0] == BAND]) == len([r for r in log if r[0] == BAND]) == 2 * classes, (log, log_no)
    if not coscheduled:
        assert log == log_no, (log, log_no)
        return
    full = (V2, cfg[0], cfg[1], 0)
    assert len(log) == len(log_no) + 1 and log.count(full) == log_no.count(full) + 1, (log, log_no)
    rest = list(log)
    rest.remove(full)
    assert sorted(rest) == sorted(log_no), (log, log_no)


def predicted(rec7, n):
    """zsw_prune_rescored by the rules of zsw_score_seed.hip / zsw_score_band.hip on the counts a records run measured (the records
    run itself never bails for fewer than 16,384 arrivals; the plain run does)"""
    no_anchor, accepted1 = int((rec7 == 0).sum()), int((rec7 == st.TIER1).sum())
    arrivals = n - no_anchor - accepted1
    if accepted1 * st.BAIL_RATIO < arrivals or arrivals < st.BAIL_BELOW:
        return n - accepted1
    return n - int((rec7 & 1).sum())


# ---- the list the seed kernel leaves: n0 on either side of a block's 128 reads, with and without a partnerless last pair -------------
@pytest.mark.parametrize("n_junk,n_clean", [(0, 2048), (1, 2048), (127, 2048), (128, 2048), (129, 2048), (257, 2048), (4097, 0)])
def test_seed_kernel_handbacks_are_scored_in_the_first_tiers_launch(world, n_junk, n_clean):
    w, ln = world, st.L
    idx = st.shuffled(np.concatenate([np.arange(n_junk), st.even_idx(w.clean0[ln], w.n_clean[ln], n_clean)]).astype(np.int64))
    res, back, log, log_no, _ = both_ways(w, read_set(w, ln, idx, f"junk{n_junk}"), "device-fixed")
    print(f"junk {n_junk} clean {n_clean}: zsw_prune_rescored {back}, log {log}")
    st.check_score(res, w.want[ln], idx, (n_junk, n_clean))
    assert back == n_junk
    check_logs(w, log, log_no, CFG[ln], True)


# ---- what the band tiers append behind n0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrivals,walks", [(2000, False), (st.BAIL_BELOW, True), (CUT - 1, False), (CUT, False), (CUT + 1, False)])
def test_the_remainder_launch_scores_exactly_what_the_band_tiers_appended(world, arrivals, walks):
    """n0 = 129; 1,000 copies (starts 0 .. 137, so that the arrival read over sorts behind every other anchored read). 2,000 arrivals:
    fewer than 16,384, the second tier hands them back unwalked; 16,384: it walks them and appends what it cannot prove; 49,151 ..
    49,153: more than 40 per read the first tier accepted, handed back unwalked — the remainder on either side of the first cut of
    the gated launches, which must choose by the remainder and not by the whole list (49,280 .. 49,282)."""
    w, ln = world, st.L
    idx = st.shuffled(np.concatenate([np.arange(129), st.even_idx(w.clean0[ln], 138, 1000), st.even_idx(w.arr0, w.n_arr, arrivals, odd_last=w.n_arr - 1)]).astype(np.int64))
    rs = read_set(w, ln, idx, f"arrivals{arrivals}")
    res, back, log, log_no, _ = both_ways(w, rs, "device-fixed")
    print(f"arrivals {arrivals}: zsw_prune_rescored {back}, log {log}")
    st.check_score(res, w.want[ln], idx, arrivals)
    check_logs(w, log, log_no, CFG[ln], True)
    if not walks:
        assert back == 129 + arrivals
        return
    res2, back_rec, _, _, rec7 = both_ways(w, rs, "device-fixed", records=True)
    st.check_score(res2, w.want[ln], idx, (arrivals, "records"))
    got1, got_none = int((rec7 == st.TIER1).sum()), int((rec7 == 0).sum())
    assert (got1, got_none, len(idx) - got1 - got_none) == (1000, 129, arrivals)
    assert int(((rec7 >> 8) == 48).sum()) == arrivals  # the second tier walked them
    assert back == back_rec == len(idx) - int((rec7 & 1).sum())


# ---- the edges of the four-lane configurations; 153 bases take eight lanes and the launches as they were ------------------------------
@pytest.mark.parametrize("ln", [24, 76, 77, 152, 153])
def test_read_lengths_at_the_edges_of_the_four_lane_configurations(world, ln):
    w = world
    idx = st.shuffled(np.concatenate([np.arange(129), st.even_idx(w.clean0[ln], w.n_clean[ln], 2048)]).astype(np.int64))
    rs = read_set(w, ln, idx, f"len{ln}")
    res, back, log, log_no, _ = both_ways(w, rs, "device-fixed")
    st.check_score(res, w.want[ln], idx, ln)
    res2, back_rec, _, _, rec7 = both_ways(w, rs, "device-fixed", records=True)
    st.check_score(res2, w.want[ln], idx, (ln, "records"))
    print(f"length {ln}: zsw_prune_rescored {back} (with records {back_rec}), no anchor {int((rec7 == 0).sum())}, accepted by tier 1 {int((rec7 == st.TIER1).sum())}, log {log}")
    assert int((rec7 == 0).sum()) >= 129
    assert back == predicted(rec7, len(idx)) and back_rec == len(idx) - int((rec7 & 1).sum())
    check_logs(w, log, log_no, CFG[ln], ln <= 152)


def test_ragged_batch_of_two_length_classes_keeps_one_n0_per_class(world):
    """100-base class: 200 junk + 1,024 copies; 150-base class: 129 junk + 2,048 copies, interleaved at random. Each class has its
    own counter and its own n0."""
    w = world
    short = st.shuffled(np.concatenate([np.arange(200), st.even_idx(w.clean0[100], 128, 1024)]).astype(np.int64), seed=2)
    long_ = st.shuffled(np.concatenate([np.arange(129), st.even_idx(w.clean0[150], w.n_clean[150], 2048)]).astype(np.int64), seed=4)
    n = len(short) + len(long_)
    is_long = np.zeros(n, dtype=bool)
    is_long[np.random.default_rng(3).permutation(n)[:len(long_)]] = True
    lens = np.where(is_long, 150, 100).astype(np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = np.empty(int(off[-1]), dtype=np.uint8)
    at = off[:-1].astype(np.int64)
    flat[(at[is_long][:, None] + np.arange(150)).reshape(-1)] = w.pool[150][long_].reshape(-1)
    flat[(at[~is_long][:, None] + np.arange(100)).reshape(-1)] = w.pool[100][short].reshape(-1)
    rs = ah.ReadSet("ragged", w.ref, np.empty(n), 0, np.zeros(n, dtype=np.int64), np.full(n, -1), _flat=flat, _off=off)
    res, back, log, log_no, _ = both_ways(w, rs, "device-ragged")
    for part, ln, idx in ((is_long, 150, long_), (~is_long, 100, short)):
        st.check_score({k: v[part] for k, v in res.items()}, w.want[ln], idx, ("ragged", ln))
    res2, back_rec, _, _, rec7 = both_ways(w, rs, "device-ragged", records=True)
    print(f"ragged: zsw_prune_rescored {back} (with records {back_rec}), log {log}")
    want = predicted(rec7[is_long], len(long_)) + predicted(rec7[~is_long], len(short))
    assert back == want and want >= 329
    V2 = w._lib.LAUNCH_V2
    assert len(log) == len(log_no) + 2 and all(log.count((V2, 4, c, 0)) == log_no.count((V2, 4, c, 0)) + 1 for c in (25, 38)), (log, log_no)
    assert len([r for r in log if r[0] == w._lib.LAUNCH_SEED_BAND]) == 4, log


def test_a_call_with_a_minimum_score_keeps_the_launches_as_they_were(world):
    """ZSW_OPTION_MIN_SCORE = the largest score of the 129 junk reads (not above any junk read's whole-read bound, so the seed
    kernel still hands them all back; above most of their scores): the MINS instantiations, not co-scheduled. The expectation is
    the option's contract applied to the oracle."""
    w, ln = world, st.L
    idx = st.shuffled(np.concatenate([np.arange(129), st.even_idx(w.clean0[ln], w.n_clean[ln], 2048)]).astype(np.int64))
    t_min = int(w.want[ln][0][:129].max())
    assert w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(t_min)) == 0
    try:
        res, back, log, log_no, _ = both_ways(w, read_set(w, ln, idx, "min-score"), "device-fixed")
    finally:
        assert w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(0)) == 0
    score, status, tier = (a[idx].copy() for a in w.want[ln])
    below = (status == ah.U_) | ((status == ah.S_) & (score < t_min))
    assert 0 < int(below.sum()) < 129
    score[below], status[below], tier[below] = 0, BELOW, 0
    st.check_score(res, (score, status, tier), np.arange(len(idx)), "min-score")
    assert back == 129
    check_logs(w, log, log_no, CFG[ln], False)
