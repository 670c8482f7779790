"""Slices of the co-scheduled hand-back list on side streams (zsw_handback.hpp: handback_slices; zsw_handback_split.hip;
zsw_score_seed.hip: launch_score_seeded). In a one-length score-only call of two band tiers the list the seed kernel leaves,
list[0, n0), is scored by the first tier's shared launch and — where the rule cuts them — by a head slice launched beside the sort
and a tail slice launched beside the second tier, each a plain launch of score_kernel_v2 that reads its range from device words. A
wrong bound gives no wrong score: it leaves reads unscored or scores them twice. So every call goes through the C ABI with
caller-owned arrays filled with 0xA5, EVERY read is compared with the oracle, no status may keep the fill, and every case runs again
under ZSW_DEBUG_SEED_NO_SLICES (the launches as they were) and must give the same score, status, tier and zsw_prune_rescored.

150-base reads against a 2,000-base reference. ZSW_DEBUG_SEED_TINY_SLICES makes the rule cut a tail of exactly 128 reads and, in
front of it, a head of 1 .. 128 reads, with no round kept for the shared launch (HANDBACK_TINY_*); ZSW_DEBUG_SCORE_PRUNE_ANY_SIZE
gives two tiers at these sizes. Junk reads (no 8-mer of the reference: never anchored, listed by the seed kernel) are n0; clean
copies are proved by the first tier.

Not here: a read at the packed-range limit inside a slice. seed_applicable admits a class only if maxw * max_len + 8 is below the
limit of its tables, so no read a seeded class hands back can reach the saturation worklist (zsw_score.hip says the same of
chunk_finalize_kernel); the join in front of add_count_kernel / exact32_kernel is there for the rule, and the case cannot be built."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah
import test_gpu_seed_thresholds as st

pytestmark = pytest.mark.gpu

REF_LEN, K, L, L_SHORT = 2000, st.K, 150, 100
TINY_TAIL, TINY_HEAD = 128, 128  # zsw_handback.hpp: HANDBACK_TINY_TAIL_READS, HANDBACK_TINY_HEAD_READS (HANDBACK_TINY_HEAD_MIN = 1)
LISTS = (0, 1, 127, 128, 129, 257, 4097)
OPTION_MIN_SCORE = 2
BELOW = 4


def tiny_slices(n0):
    """handback_slices() under the tiny rule: (shared, head, tail) as (first, end)"""
    tail = TINY_TAIL if n0 >= TINY_TAIL else 0
    head = min(TINY_HEAD, n0 - tail)
    s = n0 - tail - head
    return (0, s), (s, s + head), (s + head, n0)


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
    ref = ah.ACGT[np.random.default_rng(2000).integers(0, 4, REF_LEN)]
    w.ref = ref.tobytes()
    present = np.zeros(4 ** K, dtype=bool)
    present[st._kmer_codes(ref[None, :])[0]] = True
    junk, rng = [], np.random.default_rng(4321)
    while sum(len(j) for j in junk) < 4097:  # about one random read in eighty shares no 8-mer with 2,000 bases
        cand = ah.ACGT[rng.integers(0, 4, (100000, L))]
        junk.append(cand[~present[st._kmer_codes(cand)].any(axis=1)])
    junk = np.concatenate(junk)[:4097]
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    w.sc = oracle.Scoring(dna.signed_weights(), dna.mapping.index_map, -10, -1)
    w.pool, w.want, w.n_clean = {}, {}, {}
    for ln in (L, L_SHORT):
        clean = np.stack([ref[s:s + ln] for s in range(REF_LEN - ln + 1)])
        w.n_clean[ln] = len(clean)
        w.pool[ln] = np.ascontiguousarray(np.concatenate([junk[:, :ln], clean]))
        w.want[ln] = oracle.batch_score_w256(8, w.sc, w.pool[ln], w.ref, fixed_len=ln, threads=16)
    w.n_junk = len(junk)
    assert (w.want[L][1][:w.n_junk] == ah.S_).all()  # junk: a score, if a small one
    w.h = ah.new_context(_lib, w.lib, dna, -10, -1, w.ref)
    yield w
    w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(0))
    w.lib.zsw_debug_set(w.h, 0)
    w.lib.zsw_destroy(w.h)


def read_set(w, ln, idx, name):
    reads = w.pool[ln][idx]
    return ah.ReadSet(name, w.ref, reads, ln, np.zeros(len(idx), dtype=np.int64), np.full(len(idx), -1), _flat=reads.reshape(-1))


def both_ways(w, rs, pres):
    """the call with tiny slices and with the slices off: the same results, field by field, and the same count of full passes"""
    any_size = w._lib.DEBUG_SCORE_PRUNE_ANY_SIZE
    out = []
    for flags in (any_size | w._lib.DEBUG_SEED_TINY_SLICES, any_size | w._lib.DEBUG_SEED_TINY_SLICES | w._lib.DEBUG_SEED_NO_SLICES, any_size):
        assert w.lib.zsw_debug_set(w.h, flags) == 0
        try:
            out.append(st.call(w, "zsw_score_batch_from", rs, pres))
        finally:
            assert w.lib.zsw_debug_set(w.h, 0) == 0
    (res, back, log, _), (res_off, back_off, log_off, _), (res_def, back_def, log_def, _) = out
    for k in ("score", "status", "tier"):
        assert np.array_equal(res[k], res_off[k]), (rs.name, k, "differs from the call under ZSW_DEBUG_SEED_NO_SLICES")
        assert np.array_equal(res[k], res_def[k]), (rs.name, k, "differs from the call with the default thresholds")
    assert back == back_off == back_def, (rs.name, back, back_off, back_def)
    assert log_off == log_def, (rs.name, "a batch of this size grew a launch without the tiny-slice switch", log_off, log_def)
    return res, back, log, log_off


def test_the_lists_reach_every_branch_of_the_rule():
    parts = {n0: tiny_slices(n0) for n0 in LISTS}
    size = lambda r: r[1] - r[0]
    assert any(size(h) and not size(t) for _, h, t in parts.values())              # head only
    assert any(size(t) and not size(h) for _, h, t in parts.values())              # tail only
    assert any(size(t) and size(h) for _, h, t in parts.values())                  # both
    assert any((size(t) and t[0] % 2) or (size(h) and h[0] % 2) for _, h, t in parts.values())  # a boundary in the middle of a pair
    assert any(not size(s) and (size(h) or size(t)) for s, h, t in parts.values())  # nothing left to the shared launch
    assert any(size(s) and size(h) and size(t) for s, h, t in parts.values())      # all three parts


@pytest.mark.parametrize("n_junk,n_clean", [(0, 4098), (1, 4098), (127, 4098), (128, 4098), (129, 4100), (257, 8192), (4097, 4097)])
def test_every_read_of_a_sliced_list_is_scored_once(world, n_junk, n_clean):
    w = world
    idx = st.shuffled(np.concatenate([np.arange(n_junk), st.even_idx(w.n_junk, w.n_clean[L], n_clean, odd_last=w.n_clean[L] - 1)]).astype(np.int64))
    res, back, log, log_off = both_ways(w, read_set(w, L, idx, f"junk{n_junk}"), "device-fixed")
    print(f"junk {n_junk} clean {n_clean}: slices {tiny_slices(n_junk)}, zsw_prune_rescored {back}, log {log}, without slices {log_off}")
    st.check_score(res, w.want[L], idx, (n_junk, n_clean))
    assert back == n_junk
    # the head and the tail are launched whatever the list turns out to hold: two more ZSW_LAUNCH_V2 records, the head's of the
    # class's configuration, the tail's of the eight-lane row that holds 150 bases (HANDBACK_TAIL_G)
    head_rec, tail_rec = (w._lib.LAUNCH_V2, 4, 38, 0), (w._lib.LAUNCH_V2, 8, 19, 0)
    assert len(log) == len(log_off) + 2, (log, log_off)
    assert log.count(head_rec) == log_off.count(head_rec) + 1 and log.count(tail_rec) == log_off.count(tail_rec) + 1, (log, log_off)
    rest = list(log)
    rest.remove(head_rec)
    rest.remove(tail_rec)
    assert sorted(rest) == sorted(log_off), (log, log_off)


def test_a_ragged_batch_keeps_the_launches_as_they_were(world):
    """100-base class: 200 junk + 1,024 copies; 150-base class: 257 junk + 4,098 copies, interleaved at random: each class runs on a
    side stream already and plans no slice."""
    w = world
    short = st.shuffled(np.concatenate([np.arange(200), st.even_idx(w.n_junk, w.n_clean[L_SHORT], 1024)]).astype(np.int64), seed=2)
    long_ = st.shuffled(np.concatenate([np.arange(257), st.even_idx(w.n_junk, w.n_clean[L], 4098)]).astype(np.int64), seed=4)
    n = len(short) + len(long_)
    is_long = np.zeros(n, dtype=bool)
    is_long[np.random.default_rng(3).permutation(n)[:len(long_)]] = True
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.where(is_long, L, L_SHORT).astype(np.uint64), out=off[1:])
    flat = np.empty(int(off[-1]), dtype=np.uint8)
    at = off[:-1].astype(np.int64)
    flat[(at[is_long][:, None] + np.arange(L)).reshape(-1)] = w.pool[L][long_].reshape(-1)
    flat[(at[~is_long][:, None] + np.arange(L_SHORT)).reshape(-1)] = w.pool[L_SHORT][short].reshape(-1)
    rs = ah.ReadSet("ragged", w.ref, np.empty(n), 0, np.zeros(n, dtype=np.int64), np.full(n, -1), _flat=flat, _off=off)
    res, back, log, log_off = both_ways(w, rs, "device-ragged")
    for part, ln, idx in ((is_long, L, long_), (~is_long, L_SHORT, short)):
        st.check_score({k: v[part] for k, v in res.items()}, w.want[ln], idx, ("ragged", ln))
    assert back >= 457
    assert log == log_off, (log, log_off)


def test_a_call_with_a_minimum_score_keeps_the_launches_as_they_were(world):
    """ZSW_OPTION_MIN_SCORE = the largest score of 257 junk reads: the MINS instantiations, not co-scheduled, no slices. The
    expectation is the option's contract applied to the oracle."""
    w = world
    idx = st.shuffled(np.concatenate([np.arange(257), st.even_idx(w.n_junk, w.n_clean[L], 4098)]).astype(np.int64))
    t_min = int(w.want[L][0][:257].max())
    assert w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(t_min)) == 0
    try:
        res, back, log, log_off = both_ways(w, read_set(w, L, idx, "min-score"), "device-fixed")
    finally:
        assert w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(0)) == 0
    score, status, tier = (a[idx].copy() for a in w.want[L])
    below = (status == ah.U_) | ((status == ah.S_) & (score < t_min))
    assert 0 < int(below.sum()) < 257
    score[below], status[below], tier[below] = 0, BELOW, 0
    st.check_score(res, (score, status, tier), np.arange(len(idx)), "min-score")
    assert log == log_off, (log, log_off)
