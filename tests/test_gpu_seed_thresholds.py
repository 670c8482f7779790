"""The seeded pass's count-driven decisions, on their thresholds.

What a call of the seeded exact pass does is decided by counts: on the host the batch size (SEED_MIN_READS = 1,024: seeded or not;
SEED_NARROW_MIN_READS = 200,000: one band tier or two), on the device the reads that arrive at the second tier (SEED_BAIL_BELOW =
16,384), the first tier's accepted count times SEED_BAIL_RATIO = 40 against those arrivals, and the length of the hand-back list
against the cuts 49,152 and 327,680 of zsw_handback.hpp, which pick the gated score_kernel_v2 launch that scores the list. A wrong
comparison there gives no wrong score: it leaves reads unscored, and the caller's arrays keep what they held. So every call here
goes through the C ABI with caller-owned arrays filled with 0xA5, EVERY read is compared with the oracle, and zsw_prune_rescored
must equal the count the rule predicts.

The reads are built so that the counts are known: a 300-base random reference (K = 8);
  junk      150 random bases that share no 8-mer with the reference: no anchor, always handed back;
  clean     exact copies of the reference: the narrowest band proves them;
  arrivals  ref[s:s+70] + ref[s+82:s+162]: anchored on the longer piece, twelve diagonals from the other — outside the first tier's
            band (8 above, 6 below), inside the second's (25 above, 12 below);
clean and arrival reads of each start come in even numbers, so that lane partners (neighbours in anchor order) share an anchor.
The oracle scores each distinct read once; a batch is an index array into them."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import abi_helpers as ah

pytestmark = pytest.mark.gpu

L, L_SHORT, REF_LEN, K = 150, 100, 300, 8
CUTS = (49152, 327680)                 # zsw_handback.hpp: HANDBACK_CUTS
MIN_READS, NARROW_MIN_READS = 1024, 200000  # zsw_score_seed.hpp: SEED_MIN_READS, SEED_NARROW_MIN_READS
BAIL_BELOW, BAIL_RATIO = 16384, 40     # SEED_BAIL_BELOW, SEED_BAIL_RATIO
GAP_AT, GAP = 70, 12
TIER1, TIER2 = 0x101, (48 << 8) | 1    # record [7] of a read the diagonal tier / the 48-column tier accepted
UNWRITTEN = 0xA5A5A5A5


class World:
    pass


def _kmer_codes(a):
    """the 8-mers of every row of a 2-D array of ACGT bytes, two bits per base"""
    two = ((a >> 1) & 3).astype(np.uint32)  # A 0, C 1, T 2, G 3
    code = np.zeros((a.shape[0], a.shape[1] - K + 1), dtype=np.uint32)
    for j in range(K):
        code = (code << 2) | two[:, j:a.shape[1] - K + 1 + j]
    return code


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
    present[_kmer_codes(ref[None, :])[0]] = True
    cand = ah.ACGT[np.random.default_rng(12345).integers(0, 4, (100000, L))]
    junk = cand[~present[_kmer_codes(cand)].any(axis=1)]
    assert len(junk) > CUTS[0], len(junk)
    clean = np.stack([ref[s:s + L] for s in range(REF_LEN - L + 1)])
    arrivals = np.stack([np.concatenate([ref[s:s + GAP_AT], ref[s + GAP_AT + GAP:s + L + GAP]]) for s in range(REF_LEN - L - GAP + 1)])
    rng = np.random.default_rng(7)
    mutated = np.stack([np.frombuffer(ah._one_read(rng, ref, L, "diverged", i)[0], dtype=np.uint8) for i in range(2000)])
    w.pool = np.ascontiguousarray(np.concatenate([junk, clean, arrivals, mutated]))
    w.junk0, w.n_junk = 0, len(junk)
    w.clean0, w.n_clean = len(junk), len(clean)
    w.arr0, w.n_arr = w.clean0 + len(clean), len(arrivals)
    w.mut0, w.n_mut = w.arr0 + len(arrivals), len(mutated)
    # the shorter class of the ragged batch: prefixes of junk reads, copies of the reference
    w.pool_short = np.ascontiguousarray(np.concatenate([junk[:3000, :L_SHORT], np.stack([ref[s:s + L_SHORT] for s in range(128)])]))
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    w.sc = oracle.Scoring(dna.signed_weights(), dna.mapping.index_map, -10, -1)
    w.want = oracle.batch_score_w256(8, w.sc, w.pool, w.ref, fixed_len=L, threads=16)
    w.want_short = oracle.batch_score_w256(8, w.sc, w.pool_short, w.ref, fixed_len=L_SHORT, threads=16)
    st, s = w.want[1][:CUTS[0]], w.want[0][:CUTS[0]]
    assert (st == ah.S_).all() and s.min() >= 8 and s.max() < 60, (s.min(), s.max())  # junk: a score, and a small one
    w.ends = {}
    w.h = ah.new_context(_lib, w.lib, dna, -10, -1, w.ref)
    yield w
    w.lib.zsw_destroy(w.h)


# ---- batches as index arrays into the pool ------------------------------------------------------------------------------------------
def junk_idx(w, n):
    return w.junk0 + np.arange(n) % w.n_junk


def even_idx(first, n_variants, n, odd_last=None):
    """n reads over the variants first .. first + n_variants - 1, every variant an even number of times; an odd n puts the one
    read over on variant `odd_last` (the one with the largest anchor: it is the last anchored read of the sorted batch)"""
    pairs = n // 2
    per = pairs // n_variants + (np.arange(n_variants) < pairs % n_variants)
    idx = np.repeat(first + np.arange(n_variants), 2 * per)
    if n % 2:
        idx = np.append(idx, first + odd_last)
    assert len(idx) == n
    return idx


def shuffled(idx, seed=1):
    return idx[np.random.default_rng(seed).permutation(len(idx))]


def fixed_set(w, idx, name):
    reads = w.pool[idx]
    return ah.ReadSet(name, w.ref, reads, L, np.zeros(len(idx), dtype=np.int64), np.full(len(idx), -1), _flat=reads.reshape(-1))


def want_ends(w, pool, key, uniq):
    """sw_score_ends of the oracle for the distinct reads `uniq` of a pool, kept per module"""
    todo = sorted({int(u) for u in uniq if (key, int(u)) not in w.ends})
    if todo:  # oracle.score_ends with its arguments converted once: fifty thousand calls spend their time in the oracle, not in numpy
        o = w.oracle
        wts, im, a = o._sc_args(w.sc)
        ref = np.frombuffer(w.ref, dtype=np.uint8)
        fn, T, width = o.lib().zor_score_ends, o.TCODE["i16"], pool.shape[1]
        st, out = np.zeros(len(todo), dtype=np.uint32), np.zeros((len(todo), 3), dtype=np.uint64)
        refp, reflen, qlen = C.c_void_p(ref.ctypes.data), C.c_size_t(len(ref)), C.c_size_t(width)

        def one(k):
            return fn(T, 16, *a, C.c_void_p(pool.ctypes.data + todo[k] * width), qlen, refp, reflen, 1, C.c_void_p(st.ctypes.data + 4 * k), C.c_void_p(out.ctypes.data + 24 * k))

        with ThreadPoolExecutor(16) as ex:  # (the call releases the GIL; two thirds of a millisecond per read: 49,152 reads in 2 - 3 s)
            assert not any(ex.map(one, range(len(todo))))
        for k, u in enumerate(todo):
            w.ends[(key, u)] = (int(st[k]), tuple(int(x) for x in out[k]))
    return [w.ends[(key, int(u))] for u in uniq]


# ---- calls ----------------------------------------------------------------------------------------------------------------------------
def rescored(w):
    v = C.c_uint64(0)
    assert w.lib.zsw_prune_rescored(w.h, C.byref(v)) == 0
    return int(v.value)


def launches(w):
    n = C.c_uint32(0)
    assert w.lib.zsw_debug_score_launches(w.h, None, 0, C.byref(n)) == 0
    rec = np.zeros((max(1, n.value), 4), dtype=np.uint32)
    assert w.lib.zsw_debug_score_launches(w.h, C.c_void_p(rec.ctypes.data), n.value, C.byref(n)) == 0
    return [tuple(int(v) for v in r) for r in rec[:n.value]]


def call(w, entry, rs, pres, records=False):
    """One call on sentinel-filled output arrays -> (result arrays, zsw_prune_rescored, launch log, record [7] per read or None)"""
    import torch

    p = ah.Presented(w._lib, rs, pres)
    rec = None
    if records:
        rec = torch.zeros(8 * rs.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert w.lib.zsw_debug_band_records(w.h, rec.data_ptr()) == 0
    try:
        c = ah.Call(w._lib, w.lib, w.h, ah.ENTRY[entry], p).run()
        assert c.rc == 0, w.lib.zsw_last_error_string(w.h).decode()
        torch.cuda.synchronize()
        back, log = rescored(w), launches(w)
    finally:
        if records:
            assert w.lib.zsw_debug_band_records(w.h, None) == 0
    res = {k: a.data() for k, a in c.out.items()}
    assert all(a.guards_intact() for a in c.out.values()), (entry, "guard entries were written")
    return res, back, log, (rec.cpu().numpy().reshape(rs.n, 8)[:, 7] if records else None)


def check_score(res, want, idx, what):
    """every read of a zsw_score_batch_from call against the oracle's (score, status, tier) of its pool entry"""
    unscored = int((res["status"] == ah.FILL).sum())
    assert unscored == 0, (what, f"{unscored} of {len(idx)} reads were never scored: their statuses are still the caller's fill")
    for k, field in enumerate(("score", "status", "tier")):
        bad = np.nonzero(res[field] != want[k][idx])[0]
        assert len(bad) == 0, (what, field, f"{len(bad)} reads differ, first {bad[:5]}: got {res[field][bad[:5]]}, want {want[k][idx][bad[:5]]}")


def check_ends(res, ends, what):
    unscored = int((res["status"] == ah.FILL).sum())
    assert unscored == 0, (what, f"{unscored} of {len(ends)} reads were never scored: their statuses are still the caller's fill")
    st = np.array([e[0] for e in ends], dtype=np.uint8)
    assert np.array_equal(res["status"], st), what
    some = st == ah.S_
    for k, field in enumerate(("score", "ref_end", "query_end")):
        v = np.array([e[1][k] for e in ends], dtype=np.uint32)
        bad = np.nonzero(some & (res[field] != v))[0]
        assert len(bad) == 0, (what, field, f"{len(bad)} reads differ, first {bad[:5]}: got {res[field][bad[:5]]}, want {v[bad[:5]]}")
        assert not (res[field] == UNWRITTEN).any(), (what, field, "entries of reads without a score were never written")


# ---- A. the gates of the hand-back launches -----------------------------------------------------------------------------------------
GATE_COUNTS = [c + d for c in CUTS for d in (-1, 0, 1)]


@pytest.mark.parametrize("n_clean", [0, 2048])
@pytest.mark.parametrize("n_junk", GATE_COUNTS)
def test_handback_list_on_either_side_of_a_cut_is_scored(world, n_junk, n_clean):
    """A hand-back list of exactly cut - 1, cut and cut + 1 reads, alone in the batch (n_items = count: the list cannot be longer)
    and with 2,048 reads the band proves (n_items > count). With the launch loop as it was before handback_plan (a range launched
    only if n_items > lo) the batch of 49,152 junk reads alone came back with all 49,152 statuses still 0xA5, as did the ends call
    and the ragged class below: one launch, (32,5) with gate [0, 49,152), where there are two now."""
    w = world
    idx = shuffled(np.concatenate([junk_idx(w, n_junk), even_idx(w.clean0, w.n_clean, n_clean)]))
    res, back, log, _ = call(w, "zsw_score_batch_from", fixed_set(w, idx, "gate"), "device-fixed")
    print(f"junk {n_junk} clean {n_clean}: zsw_prune_rescored {back}, V2 launches {[r for r in log if r[0] == w._lib.LAUNCH_V2]}")
    check_score(res, w.want, idx, (n_junk, n_clean))
    assert back == n_junk


def test_handback_list_of_exactly_49152_reads_through_the_ends_call(world):
    """mode 2 (zsw_score_ends_batch): n_items = count = 49,152"""
    w = world
    idx = junk_idx(w, CUTS[0])
    res, back, log, _ = call(w, "zsw_score_ends_batch", fixed_set(w, idx, "gate-ends"), "device-fixed")
    print(f"ends, junk {CUTS[0]}: zsw_prune_rescored {back}, V2 launches {[r for r in log if r[0] == w._lib.LAUNCH_V2]}")
    check_ends(res, want_ends(w, w.pool, "L", idx), "ends")
    assert back == CUTS[0]


@pytest.mark.parametrize("entry", ["zsw_score_batch_from", "zsw_score_ends_batch"])
def test_length_class_of_exactly_49152_handed_back_reads_in_a_ragged_batch(world, entry):
    """The 150-base class holds 49,152 junk reads and nothing else; the 100-base class 3,000 junk reads and 1,024 copies."""
    w = world
    short = shuffled(np.concatenate([np.arange(3000), even_idx(3000, 128, 1024)]), seed=2)
    n_long, n = CUTS[0], CUTS[0] + len(short)
    is_long = np.zeros(n, dtype=bool)
    is_long[np.random.default_rng(3).permutation(n)[:n_long]] = True
    lens = np.where(is_long, L, L_SHORT).astype(np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = np.empty(int(off[-1]), dtype=np.uint8)
    long_idx = junk_idx(w, n_long)
    at = off[:-1].astype(np.int64)
    flat[(at[is_long][:, None] + np.arange(L)).reshape(-1)] = w.pool[long_idx].reshape(-1)
    flat[(at[~is_long][:, None] + np.arange(L_SHORT)).reshape(-1)] = w.pool_short[short].reshape(-1)
    rs = ah.ReadSet("ragged", w.ref, np.empty(n), 0, np.zeros(n, dtype=np.int64), np.full(n, -1), _flat=flat, _off=off)
    res, back, log, _ = call(w, entry, rs, "device-ragged")
    print(f"{entry}, ragged: zsw_prune_rescored {back}, V2 launches {[r for r in log if r[0] == w._lib.LAUNCH_V2]}")
    if entry == "zsw_score_batch_from":
        for part, want, idx in ((is_long, w.want, long_idx), (~is_long, w.want_short, short)):
            check_score({k: v[part] for k, v in res.items()}, want, idx, ("ragged", int(part.sum())))
    else:
        ends = [None] * n
        for part, e in ((is_long, want_ends(w, w.pool, "L", long_idx)), (~is_long, want_ends(w, w.pool_short, "S", short))):
            for i, v in zip(np.nonzero(part)[0], e):
                ends[i] = v
        check_ends(res, ends, "ragged ends")
    assert back == n_long + 3000


# ---- B. the switches the host decides by the batch size -----------------------------------------------------------------------------
def predicted_rescored(rec7, n):
    """The rule of zsw_score_seed.hip / zsw_score_band.hip on the counts a records run measured (two tiers: the records run itself
    never bails for fewer than 16,384 arrivals, the plain run does)."""
    no_anchor, accepted1 = int((rec7 == 0).sum()), int((rec7 == TIER1).sum())
    arrivals = n - no_anchor - accepted1
    if n >= NARROW_MIN_READS and (accepted1 * BAIL_RATIO < arrivals or arrivals < BAIL_BELOW):
        return n - accepted1
    return n - int((rec7 & 1).sum())


@pytest.mark.parametrize("n,band_launches", [(MIN_READS - 1, 0), (MIN_READS, 1), (NARROW_MIN_READS - 1, 1), (NARROW_MIN_READS, 2)])
def test_batch_size_switches_the_seeded_pass_and_its_second_tier(world, n, band_launches):
    """1,023 reads: no seeded pass; 1,024 and 199,999: one band tier; 200,000: two. A third each of copies, reads with 3 - 12 %
    substitutions and junk; the hand-backs are those the band records of a second run of the same batch show."""
    w = world
    third = n // 3 // 2 * 2
    n_junk = n - 2 * third
    idx = shuffled(np.concatenate([even_idx(w.clean0, w.n_clean, third), w.mut0 + np.arange(third) % w.n_mut, junk_idx(w, n_junk)]))
    rs = fixed_set(w, idx, "switch")
    res, back, log, _ = call(w, "zsw_score_batch_from", rs, "device-fixed")
    check_score(res, w.want, idx, n)
    band = [r for r in log if r[0] == w._lib.LAUNCH_SEED_BAND]
    assert len(band) == band_launches, log
    if band_launches == 0:
        assert back == 0 and not [r for r in log if r[0] == w._lib.LAUNCH_SEED_WINDOW], log
        return
    res2, back2, _, rec7 = call(w, "zsw_score_batch_from", rs, "device-fixed", records=True)
    check_score(res2, w.want, idx, (n, "records"))
    print(f"n {n}: zsw_prune_rescored {back} (with records {back2}), no anchor {int((rec7 == 0).sum())}, accepted by tier 1 {int((rec7 == TIER1).sum())}, by any {int((rec7 & 1).sum())}")
    # (the band walked every read but the junk, and some diverged ones that kept no anchor; it proved the copies at least)
    assert n_junk <= int((rec7 == 0).sum()) < n_junk + third // 4 and int((rec7 & 1).sum()) >= third
    assert back == predicted_rescored(rec7, n)


# ---- C. the second tier's rules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accepted1,arrivals,walks", [(2048, BAIL_BELOW, True), (2048, BAIL_BELOW - 1, False),
                                                      (410, 410 * BAIL_RATIO, True), (410, 410 * BAIL_RATIO + 1, False)])
def test_second_tier_walks_or_bails_on_its_thresholds(world, accepted1, arrivals, walks):
    """200,000 reads: `accepted1` copies (the first tier accepts them), `arrivals` reads with a twelve-base deletion (the first tier
    cannot prove them, the second can), junk for the rest. The second tier hands its arrivals back unwalked if they are fewer than
    16,384 or more than 40 per read the first tier accepted. The first run measures the counts through the band records and must
    find exactly the intended ones; the second, without records, must count the hand-backs its side of the rule predicts."""
    w = world
    n = NARROW_MIN_READS
    n_junk = n - accepted1 - arrivals
    # copies from starts 0 .. 137 only: the arrival read over (start 138, anchor 150) then sorts behind every other anchored read
    idx = shuffled(np.concatenate([even_idx(w.clean0, 138, accepted1), even_idx(w.arr0, w.n_arr, arrivals, odd_last=w.n_arr - 1), junk_idx(w, n_junk)]))
    rs = fixed_set(w, idx, "tiers")
    res, back_rec, _, rec7 = call(w, "zsw_score_batch_from", rs, "device-fixed", records=True)
    check_score(res, w.want, idx, ("records", accepted1, arrivals))
    got1, got_none, got2, any_ok = int((rec7 == TIER1).sum()), int((rec7 == 0).sum()), int((rec7 == TIER2).sum()), int((rec7 & 1).sum())
    walked2 = int(((rec7 >> 8) == 48).sum())
    print(f"accepted1 {got1}, no anchor {got_none}, arrivals {n - got_none - got1}; records run: second tier walked {walked2}, accepted {got2}, rescored {back_rec}")
    assert got1 == accepted1 and got_none == n_junk and n - got_none - got1 == arrivals
    # with records the second tier has no floor of 16,384 arrivals: it walks unless the ratio rule bails
    ratio_bails = accepted1 * BAIL_RATIO < arrivals
    assert walked2 == (0 if ratio_bails else arrivals)
    assert back_rec == n - any_ok
    if not ratio_bails:
        assert got2 >= 1000  # so that the two sides of the rule predict different counts
    res, back, log, _ = call(w, "zsw_score_batch_from", rs, "device-fixed")
    check_score(res, w.want, idx, (accepted1, arrivals))
    print(f"plain run: zsw_prune_rescored {back}")
    assert len([r for r in log if r[0] == w._lib.LAUNCH_SEED_BAND]) == 2, log
    assert walks == (not ratio_bails and arrivals >= BAIL_BELOW)
    assert back == (n - any_ok if walks else n - accepted1)
