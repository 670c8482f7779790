"""The row-chunked full pass over the reads the seeded pass hands back (zsw_score.hip: seed_items; zsw_score_v2.hpp:
ScoreArgsV2::chunk_rows), at its chunk edges and at the thresholds that switch it on.

Chunk k of a read walks reference rows [kB - V, (k + 1)B) from a zero state and folds (score, first row, first column) into the
read's 64-bit key; chunk_finalize_kernel turns the keys into the outputs. A wrong boundary there gives a plausible but lower
score, or the right score with another end row, so every comparison is equality with the oracle, on reads built to sit on the
edges: tests/chunk_edge_reads.py builds them — alignments that end on the last row a chunk owns and on the first, that cross a
boundary with the longest span the scheme lets one build, that hold the same maximum in several chunks or in two columns of one
row — and derives B, V, the number of chunks and whether a call is chunked at all from the scheme, the read length and the
reference length alone; tests/test_chunk_edge_reads.py holds the reads to the oracle on the CPU. Every edge read is K-mer-free,
so the seed kernel finds no anchor and hands it back; 1,024 exact copies of the reference per class (which the band proves) make
the call a seeded one.

Every call goes through the C ABI with caller-owned arrays filled with 0xA5 and asserts: no status keeps the fill and the guard
entries are intact; every read equals the oracle; the same call under ZSW_DEBUG_NO_ROW_CHUNKS gives identical arrays;
zsw_prune_rescored is the number of K-mer-free reads; the launch log holds (ZSW_LAUNCH_ROW_CHUNKS, B, V, chunks) with the
generator's numbers once per chunked class, directly in front of a ZSW_LAUNCH_V2 record, and no such record under the flag or
where the rule says the call is not chunked. A call that quietly fell back to whole rows fails here."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah
import chunk_edge_reads as cer
import test_gpu_seed_thresholds as st

pytestmark = pytest.mark.gpu

N_COPIES = 1024
OPTION_MIN_SCORE, BELOW = 2, 4
ENTRIES = ("zsw_score_batch_from", "zsw_score_ends_batch")


class GpuWorld:
    pass


@pytest.fixture(scope="module")
def worlds(oracle):
    """name -> the generator's world with a context of its own, the oracle's (score, status, tier) of every distinct read"""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib

    built = {}

    def get(name):
        if name not in built:
            w = GpuWorld()
            w._lib, w.lib, w.oracle, w.za = _lib, _lib.load(), oracle, zoe_amd
            w.cw = cer.world(name)
            ma, mi, go, ge = w.cw.scheme
            w.dna = zoe_amd.WeightMatrix.new_dna_matrix(ma, mi, b"N")
            w.sc = oracle.Scoring(w.dna.signed_weights(), w.dna.mapping.index_map, go, ge)
            w.ref, w.ends = w.cw.ref, {}
            w.want = [oracle.batch_score_w256(8, w.sc, cs.pool, w.ref, fixed_len=cs.length, threads=16) for cs in w.cw.classes]
            w.h = ah.new_context(_lib, w.lib, w.dna, go, ge, w.ref)
            built[name] = w
        return built[name]

    yield get
    for w in built.values():
        w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(0))
        w.lib.zsw_debug_set(w.h, 0)
        w.lib.zsw_destroy(w.h)


def batch_of(w):
    """(read set, presentation, per class: (mask of its reads in the batch, indices into its pool), K-mer-free reads per class).
    Per class: every edge read, junk to an ODD number of K-mer-free reads (the last lane pair of the hand-back launch is half
    empty), 1,024 copies; shuffled, and the classes of the ragged world interleaved at random."""
    parts = []
    for cs in w.cw.classes:
        n_junk = 100 + (cs.n_edges % 2 == 0)
        parts.append((cs, cer.batch_indices(cs, n_junk, N_COPIES), cs.n_edges + n_junk))
    if not w.cw.ragged:
        cs, idx, free = parts[0]
        reads = cs.pool[idx]
        rs = ah.ReadSet(w.cw.name, w.ref, reads, cs.length, np.zeros(len(idx), dtype=np.int64), np.full(len(idx), -1), _flat=reads.reshape(-1))
        return rs, "device-fixed", [(np.ones(len(idx), dtype=bool), idx)], [free]
    n = sum(len(idx) for _, idx, _ in parts)
    cls = np.repeat(np.arange(len(parts)), [len(idx) for _, idx, _ in parts])[np.random.default_rng(3).permutation(n)]
    lens = np.array([cs.length for cs, _, _ in parts], dtype=np.uint64)[cls]
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = np.empty(int(off[-1]), dtype=np.uint8)
    at = off[:-1].astype(np.int64)
    masks = []
    for k, (cs, idx, _) in enumerate(parts):
        m = cls == k
        flat[(at[m][:, None] + np.arange(cs.length)).reshape(-1)] = cs.pool[idx].reshape(-1)
        masks.append((m, idx))
    rs = ah.ReadSet(w.cw.name, w.ref, np.empty(n), 0, np.zeros(n, dtype=np.int64), np.full(n, -1), _flat=flat, _off=off)
    return rs, "device-ragged", masks, [free for _, _, free in parts]


def call_flagged(w, entry, rs, pres, flags):
    assert w.lib.zsw_debug_set(w.h, flags) == 0
    try:
        return st.call(w, entry, rs, pres)
    finally:
        assert w.lib.zsw_debug_set(w.h, 0) == 0


def check_oracle(w, entry, res, masks, what):
    if entry == "zsw_score_batch_from":
        for k, (m, idx) in enumerate(masks):
            st.check_score({f: v[m] for f, v in res.items()}, w.want[k], idx, (what, w.cw.classes[k].length))
        return
    ends = [None] * len(res["status"])
    for k, (m, idx) in enumerate(masks):
        for i, v in zip(np.nonzero(m)[0], st.want_ends(w, w.cw.classes[k].pool, k, idx)):
            ends[i] = v
    st.check_ends(res, ends, what)


def check_records(w, log, expected, mode, what):
    """the ZSW_LAUNCH_ROW_CHUNKS records of a launch log: exactly `expected`, each directly in front of a score_kernel_v2 record of
    the call's mode"""
    RC, V2 = w._lib.LAUNCH_ROW_CHUNKS, w._lib.LAUNCH_V2
    at = [i for i, r in enumerate(log) if r[0] == RC]
    assert sorted(log[i] for i in at) == sorted(expected), (what, log)
    for i in at:
        assert i + 1 < len(log) and log[i + 1][0] == V2 and log[i + 1][3] == mode, (what, log)


def expected_records(w):
    return [(w._lib.LAUNCH_ROW_CHUNKS, cs.p.B, cs.p.V, cs.p.chunks) for cs in w.cw.classes if cs.p.chunked]


# the numbers of the issue's table, against which the generator's own are held before anything runs: (B, V, chunks) per chunked class
TABLE = {"A": [(2048, 452, 5)], "A0": [(2048, 452, 4)], "A-": [], "B": [(2048, 452, 5)], "C": [(2048, 334, 5)], "D": [(4808, 1202, 2)], "D-": [],
         "D+": [(4808, 1202, 3)], "E": [(2048, 458, 5), (3656, 914, 3)], "F": []}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(cer.WORLDS))
def test_edge_reads_of_a_world_equal_the_oracle_and_the_log_shows_the_chunks(worlds, name, entry):
    """A, A0, A-: a reference of 8,193, 8,192 and 8,191 rows — five chunks the last of which owns one row, four chunks exactly,
    not chunked. B: gap_open 2, the reads that span 330 of V = 452 rows. C: gap_extend 5, V = 151 + floor(906 / 5) + 2. D, D-,
    D+: 400-base reads, B = 4,808 (not a power of two), 2 B = 9,616 on either side: two chunks, not chunked, three chunks the last
    of which owns one row. E: one ragged call of three classes (capacities 152, 304, 608) — B 2,048 and 3,656 on concurrent
    streams, sharing one key array, and a class that is not chunked (2 B > 8,193) beside them — once more without side streams.
    F: gap_extend 0, never chunked."""
    w = worlds(name)
    assert [r[1:] for r in expected_records(w)] == TABLE[name]
    rs, pres, masks, free = batch_of(w)
    mode = 0 if entry == "zsw_score_batch_from" else 2
    res, back, log, _ = st.call(w, entry, rs, pres)
    print(f"{name} {entry}: {rs.n} reads, zsw_prune_rescored {back} (K-mer-free {free}), log {log}")
    check_oracle(w, entry, res, masks, name)
    assert back == sum(free), (name, back, free)
    check_records(w, log, expected_records(w), mode, name)
    res_no, back_no, log_no, _ = call_flagged(w, entry, rs, pres, w._lib.DEBUG_NO_ROW_CHUNKS)
    for f in res:
        assert np.array_equal(res[f], res_no[f]), (name, f, "differs from the call under ZSW_DEBUG_NO_ROW_CHUNKS")
    assert back_no == back
    check_records(w, log_no, [], mode, (name, "ZSW_DEBUG_NO_ROW_CHUNKS"))
    if w.cw.ragged:
        res_1, back_1, log_1, _ = call_flagged(w, entry, rs, pres, w._lib.DEBUG_NO_SIDE_STREAMS)
        for f in res:
            assert np.array_equal(res[f], res_1[f]), (name, f, "differs from the call under ZSW_DEBUG_NO_SIDE_STREAMS")
        assert back_1 == back
        check_records(w, log_1, expected_records(w), mode, (name, "ZSW_DEBUG_NO_SIDE_STREAMS"))


def test_ranges_and_alignments_of_the_edge_reads_through_the_python_api(worlds, oracle):
    """World A through LocalProfilesBatch: sw_score_ranges_from_i8 (its forward pass is the mode-2 chunked launch) and
    sw_align_from_i8 (its first pass the mode-1 one), every distinct edge read against oracle.cascade_score_ranges /
    cascade_align; both calls must show the chunk record."""
    import torch

    w = worlds("A")
    za, cs = w.za, w.cw.classes[0]
    ctx = za.SwContext.get(0)
    idx = cer.batch_indices(cs, 101, N_COPIES)
    reads = np.ascontiguousarray(cs.pool[idx])
    prof = za.LocalProfilesBatch.new_with_w256(za.ReadBatch.from_fixed(torch.from_numpy(reads.reshape(-1)).cuda(), cs.length), w.dna, w.cw.scheme[2], w.cw.scheme[3])
    rec = expected_records(w)[0]
    rg = prof.sw_score_ranges_from_i8(za.SeqSrc.Reference(w.ref))
    assert ctx.debug_score_launches().count(rec) == 1, ctx.debug_score_launches()
    al = prof.sw_align_from_i8(za.SeqSrc.Reference(w.ref))
    assert ctx.debug_score_launches().count(rec) == 1, ctx.debug_score_launches()
    where = {int(u): int(np.nonzero(idx == u)[0][0]) for u in range(cs.n_edges)}
    for u, e in enumerate(cs.edges):
        i = where[u]
        o_st, o_s, o_rr, o_qr, o_t = oracle.cascade_score_ranges(8, 256, w.sc, e.seq, w.ref)
        assert o_st == ah.S_ and o_rr == (e.start, e.end), e.tag
        got = (int(rg.status[i]), int(rg.score[i]), (int(rg.ref_start[i]), int(rg.ref_end[i])), (int(rg.query_start[i]), int(rg.query_end[i])), int(rg.tier[i]))
        assert got == (o_st, o_s, o_rr, o_qr, o_t), (e.tag, got)
        want, _tier = oracle.cascade_align(8, 256, w.sc, e.seq, w.ref)
        assert want.status == ah.S_ and al.key(i) == want.key(), (e.tag, al.key(i), want.key())


def test_a_minimum_score_between_two_designed_scores(worlds):
    """World A with ZSW_OPTION_MIN_SCORE = 100: above the reads of the long plan (58) and X + X (85), below those of the duplicated
    stretch (118 and more), which therefore still come out of the chunks with their scores. The expectation is the option's
    contract applied to the oracle."""
    w = worlds("A")
    cs = w.cw.classes[0]
    rs, pres, masks, free = batch_of(w)
    idx = masks[0][1]
    score, status, tier = (a[idx].copy() for a in w.want[0])
    t_min = 100
    edge_scores = w.want[0][0][:cs.n_edges]
    assert (edge_scores < t_min).sum() >= 8 and (edge_scores >= t_min).sum() >= 3, edge_scores
    below = (status == ah.U_) | ((status == ah.S_) & (score < t_min))
    score[below], status[below], tier[below] = 0, BELOW, 0
    assert w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(t_min)) == 0
    try:
        res, back, log, _ = st.call(w, "zsw_score_batch_from", rs, pres)
        res_no, back_no, log_no, _ = call_flagged(w, "zsw_score_batch_from", rs, pres, w._lib.DEBUG_NO_ROW_CHUNKS)
    finally:
        assert w.lib.zsw_set_option(w.h, OPTION_MIN_SCORE, C.c_int64(0)) == 0
    print(f"minimum score {t_min}: zsw_prune_rescored {back}, log {log}")
    st.check_score(res, (score, status, tier), np.arange(len(idx)), "min-score")
    for f in res:
        assert np.array_equal(res[f], res_no[f]), f
    # (the seed kernel settles a K-mer-free read whose whole-read bound is below the minimum itself: fewer hand-backs, not more)
    assert int((edge_scores >= t_min).sum()) <= back == back_no <= free[0]
    check_records(w, log, expected_records(w), 0, "min-score")
    check_records(w, log_no, [], 0, "min-score, ZSW_DEBUG_NO_ROW_CHUNKS")
