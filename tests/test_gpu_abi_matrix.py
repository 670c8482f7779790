"""Every entry point of the C ABI (include/zoe_sw.h) with every presentation of a batch the ABI allows.

The product's caller holds reads in HOST memory, fixed-length, ragged or packed four bits to a base, and may pass a stream of its
own; the rest of the GPU suite hands over device tensors on the default stream. Here the same reads go through
device / host x fixed / ragged / packed4 x (NULL stream, a non-blocking stream of the test's own): every output array must be
byte-identical to the `device-fixed` call on the NULL stream (`device-ragged` for the truly ragged set), and that one call is
compared with the oracle. Host and device output arrays carry 64 guard entries in front and behind; the alignment calls go
through the ciglet capacity protocol (0 with null arrays, total - 1, total) every time.

Read sets (abi_helpers.mixed_set): reads near the reference, 3-12 % diverged, with one and with several indels, tie-rich and
low-complexity reads, lower case / U / N / IUPAC bytes, unrelated reads, all-N reads; L = 150 and L = 151 (the last packed byte
holds one base), a ragged set (1..400 bases, some empty), prefixes of 1, 2 and 65 reads (below the seeded threshold), and one set
scored at T = i8 so that OVERFLOWED crosses the boundary. test_read_sets_meet_conditions asserts from the oracle's answers that
the sets are not trivial."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah
from abi_helpers import CLASSES, ENTRIES, ENTRY, PRESENTATIONS, S_, O_, U_, E_

pytestmark = pytest.mark.gpu

FIXED_SETS = ("L150", "L151")
TINY = (1, 2, 65)
STREAMS = ("null-stream", "own-stream")
THRESHOLD = 0.05  # of the sneaky-snake filter


class Env:
    pass


@pytest.fixture(scope="module")
def env(oracle):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib, synth

    e = Env()
    e.za, e._lib, e.lib, e.oracle = zoe_amd, _lib, _lib.load(), oracle
    e.ref = synth.reference_host(2000)
    e.dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    e.sc = oracle.Scoring(e.dna.signed_weights(), e.dna.mapping.index_map, -10, -1)
    e.h = ah.new_context(_lib, e.lib, e.dna, -10, -1, e.ref, pseq=e.ref)  # shared role: the profile sequence is the reference
    e.sets = {
        "L150": ah.mixed_set("L150", e.ref, 3000, 150, 150),
        "L151": ah.mixed_set("L151", e.ref, 3001, 151, 151),
        "ragged": ah.mixed_set("ragged", e.ref, 3000, 0, 7),
        "i8": ah.mixed_set("i8", e.ref, 3000, 150, 8, T="i8", lanes=32),
    }
    for n in TINY:
        e.sets[f"tiny{n}"] = e.sets["L151"].subset(n, f"tiny{n}")
    e.own = torch.cuda.Stream()
    e.presented, e.base, e.full_align = {}, {}, {}
    yield e
    e.presented.clear()
    e.base.clear()
    e.lib.zsw_destroy(e.h)


def presented(env, set_name, pres):
    key = (set_name, pres)
    if key not in env.presented:
        env.presented[key] = ah.Presented(env._lib, env.sets[set_name], pres, env.lib, env.h, env.dna.mapping.index_map)
    return env.presented[key]


def base_pres(set_name):
    return "device-ragged" if set_name == "ragged" else "device-fixed"


def baseline(env, entry, set_name):
    """the entry point's answer for the device-resident batch on the NULL stream, once per module"""
    key = (entry.name, set_name)
    if key not in env.base:
        env.base[key] = ah.Call(env._lib, env.lib, env.h, entry, presented(env, set_name, base_pres(set_name))).run().collect()
    return env.base[key]


def stream_of(env, which):
    return None if which == "null-stream" else env.own


def full_align(env, set_name):
    """oracle: sw_align at the set's <T, N> of EVERY read against the reference (SeqSrc::Reference), once per module"""
    if set_name not in env.full_align:
        rs, o = env.sets[set_name], env.oracle

        def one(r):
            try:
                return o.align(rs.T, rs.lanes, env.sc, r, env.ref)
            except o.ProfileError:
                return o.Aln(status=E_)

        env.full_align[set_name] = ah.pmap(one, rs.reads)
    return env.full_align[set_name]


# ---- the sets are not trivial ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("set_name", ["L150", "L151", "ragged", "i8"])
def test_read_sets_meet_conditions(env, set_name):
    rs, o = env.sets[set_name], env.oracle
    al = full_align(env, set_name)
    st = np.array([a.status for a in al])
    assert (st == S_).any() and (st == U_).any(), np.bincount(st, minlength=4)
    if set_name == "i8":
        assert (st == O_).sum() > rs.n // 10 and (st == S_).sum() > rs.n // 10, np.bincount(st, minlength=4)
        return
    if set_name == "ragged":
        assert (st == E_).sum() >= 30 and min(len(r) for r in rs.reads) == 0 and max(len(r) for r in rs.reads) > 380
    some = st == S_
    ins = np.array(["I" in a.cigar for a in al])[some].mean()
    dele = np.array(["D" in a.cigar for a in al])[some].mean()
    assert ins >= 0.05 and dele >= 0.05, (ins, dele)
    # a maximum in more than one cell: the read-as-profile rule (first reference row, then first read column) and the shared
    # role's (first read position, then first sequence position) pick different cells
    ties = [rs.reads[i] for i in np.nonzero(rs.cls == CLASSES.index("ties"))[0] if rs.reads[i]]

    def two_rules(r):
        s1, (_a, re1, qe1) = o.score_ends("i16", 16, env.sc, r, env.ref)
        s2, (_b, re2, qe2) = o.score_ends("i16", 16, env.sc, env.ref, r)
        return s1 == S_ and s2 == S_ and (re1, qe1) != (qe2, re2)

    assert sum(ah.pmap(two_rules, ties)) >= 5


# ---- device-fixed against the oracle -----------------------------------------------------------------------------------------

def _got_key(entry, res, i):
    st = int(res["status"][i])
    if entry.kind == "align":
        k = ah.aln_key(res, i)
    elif st != S_:
        k = (st,)
    elif entry.kind == "ends":
        k = (st, int(res["score"][i]), int(res["ref_end"][i]), int(res["query_end"][i]))
    else:
        k = (st, int(res["score"][i]), (int(res["ref_start"][i]), int(res["ref_end"][i])), (int(res["query_start"][i]), int(res["query_end"][i])))
    return k + ((int(res["tier"][i]),) if entry.cascade and st == S_ else ())


def _want_key(env, entry, rs, read):
    """the oracle's answer for one read, in the shape of _got_key"""
    o, sc = env.oracle, env.sc
    prof, other = (env.ref, read) if entry.shared else (read, env.ref)
    empty = (U_,) if entry.shared else (E_,)  # an empty read is an empty `reference` in the shared role, a ProfileError otherwise
    if len(read) == 0:
        return (empty[0], 0, (0, 0), (0, 0), "", 0, 0) if entry.kind == "align" else empty
    tier = ()
    if entry.kind == "ends":
        st, (s, re_, qe) = o.score_ends(rs.T, rs.lanes, sc, prof, other)
        return (st, s, re_, qe) if st == S_ else (st,)
    if entry.kind == "ranges":
        if entry.cascade:
            st, s, rr, qr, t = o.cascade_score_ranges(8, 256, sc, prof, other)
            tier = (t,)
        else:
            st, s, rr, qr = o.score_ranges(rs.T, rs.lanes, sc, prof, other)
        return (st, s, rr, qr) + tier if st == S_ else (st,)
    q = bool(entry.invert)
    if entry.threepass:
        a, *rest = o.cascade_align_3pass(8, 256, sc, prof, other, other_is_query=q) if entry.cascade else o.align_3pass(rs.T, rs.lanes, sc, prof, other, other_is_query=q)
    else:
        a, *rest = o.cascade_align(8, 256, sc, prof, other, other_is_query=q) if entry.cascade else (o.align(rs.T, rs.lanes, sc, prof, other, other_is_query=q),)
    if a.status != S_:
        return (a.status, 0, (0, 0), (0, 0), "", 0, 0)
    return a.key() + ((rest[0],) if entry.cascade else ())


def _check_scores(env, entry, rs, res):
    """score, status (and tier) of EVERY read through the batch oracle (per read for T = i8)"""
    o, sc = env.oracle, env.sc
    n = rs.n
    lens = np.array([len(r) for r in rs.reads])
    full = lens > 0
    want_st = np.full(n, U_ if entry.shared else E_, dtype=np.uint8)
    want_s, want_t = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    if not entry.cascade and rs.T == "i8":
        prs = ah.pmap(lambda r: o.score("i8", rs.lanes, sc, *((env.ref, r) if entry.shared else (r, env.ref))), rs.reads)
        want_st[:] = [p[0] for p in prs]
        want_s[:] = [p[1] for p in prs]
    else:
        keep = [r for r in rs.reads if r]
        off = np.zeros(len(keep) + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in keep], out=off[1:])
        cat = np.frombuffer(b"".join(keep), dtype=np.uint8)
        width = 8 if entry.cascade else 16
        if entry.shared:
            want_s[full], want_st[full] = o.batch_score_shared_w256(width, sc, cat, env.ref, offsets=off, threads=ah.ORACLE_THREADS)
        else:
            want_s[full], want_st[full], want_t[full] = o.batch_score_w256(width, sc, cat, env.ref, offsets=off, threads=ah.ORACLE_THREADS)
    assert np.array_equal(res["status"], want_st), np.nonzero(res["status"] != want_st)[0][:8]
    some = want_st == S_
    assert np.array_equal(res["score"][some], want_s[some]), np.nonzero(some & (res["score"] != want_s))[0][:8]
    if entry.cascade and not entry.shared:
        assert np.array_equal(res["tier"][full], want_t[full]), np.nonzero(full & (res["tier"] != want_t))[0][:8]


ORACLE_CASES = [(e.name, s) for e in ENTRIES for s in ("L150", "L151", "ragged")] + [(e.name, "i8") for e in ENTRIES if not e.cascade]


@pytest.mark.parametrize("entry_name,set_name", ORACLE_CASES, ids=[f"{e}-{s}" for e, s in ORACLE_CASES])
def test_device_batch_equals_oracle(env, entry_name, set_name):
    """`device-fixed` (`device-ragged` for the ragged set) on the NULL stream against the oracle: scores on every read, the other
    families on a fixed sample of 300 reads that holds the edge classes and the reads with gaps first; sw_align at <T, N> on
    every read."""
    entry, rs = ENTRY[entry_name], env.sets[set_name]
    res = baseline(env, entry, set_name)
    if entry.kind == "score":
        _check_scores(env, entry, rs, res)
        if entry.cascade and entry.shared:  # the batch oracle of the shared role has no tiers: the sample, per read
            idx = ah.sample_of(rs)
            want = ah.pmap(lambda i: env.oracle.cascade_score(8, 256, env.sc, env.ref, rs.reads[i]) if rs.reads[i] else (U_, 0, None), idx)
            for i, (st, s, t) in zip(idx, want):
                assert int(res["status"][i]) == st and (t is None or int(res["tier"][i]) == t), (i, st, s, t)
        return
    if entry.name == "zsw_align_batch":
        idx = np.arange(rs.n)
        want = [a.key() if a.status == S_ else (a.status, 0, (0, 0), (0, 0), "", 0, 0) for a in full_align(env, set_name)]
    else:
        idx = ah.sample_of(rs)
        assert len(idx) >= 300
        want = ah.pmap(lambda i: _want_key(env, entry, rs, rs.reads[i]), idx)
    for i, w in zip(idx, want):
        assert _got_key(entry, res, int(i)) == w, (entry.name, set_name, int(i), CLASSES[rs.cls[i]])
    if entry.kind == "align":
        # ciglets are packed in read order: the layout is part of the contract
        rec, some = res["aln"], res["status"] == S_
        nc = np.where(some, rec["n_ciglets"], 0).astype(np.uint64)
        assert int(nc.sum()) == int(res["total"][0]) == len(res["inc"])
        assert np.array_equal(rec["ciglet_offset"][some], (np.cumsum(nc) - nc)[some])


# ---- every presentation equals the device batch ------------------------------------------------------------------------------

def _matrix_cases():
    cases = []
    for e in ENTRIES:
        for s in FIXED_SETS + (("i8",) if not e.cascade else ()):
            cases += [(e.name, s, p, st) for p in PRESENTATIONS for st in STREAMS if (p, st) != ("device-fixed", "null-stream")]
        cases += [(e.name, "ragged", p, st) for p in ("device-ragged", "host-ragged") for st in STREAMS if (p, st) != ("device-ragged", "null-stream")]
        cases += [(e.name, f"tiny{n}", p, st) for n in TINY for p in ("host-fixed", "host-ragged", "host-packed4") for st in STREAMS]
    return cases


MATRIX = _matrix_cases()


@pytest.mark.parametrize("entry_name,set_name,pres,stream", MATRIX, ids=["-".join(c) for c in MATRIX])
def test_presentation_equals_device_batch(env, entry_name, set_name, pres, stream):
    entry = ENTRY[entry_name]
    got = ah.Call(env._lib, env.lib, env.h, entry, presented(env, set_name, pres), stream_of(env, stream)).run().collect()
    if set_name.startswith("tiny"):  # a prefix of L151 (below the seeded threshold: the full pass answers): the prefix of its arrays
        n, big = env.sets[set_name].n, baseline(env, entry, "L151")
        want = {k: v[:n] for k, v in big.items() if k not in ("inc", "op", "total")}
        if entry.kind == "align":
            t = int(np.where(big["status"][:n] == S_, big["aln"]["n_ciglets"][:n], 0).sum())
            want.update(inc=big["inc"][:t], op=big["op"][:t], total=np.array([t], dtype=np.uint64))
    else:
        want = baseline(env, entry, set_name)
    ah.assert_same(got, want, f"{entry_name} {set_name} {pres} {stream}")


# ---- the pre-alignment filter ------------------------------------------------------------------------------------------------

def _windows(rs, R):
    """candidate windows: where the read was cut from (elsewhere for reads from nowhere), mostly of the read's length, some a few
    bases off and some so far off that the filter answers None"""
    rng = np.random.default_rng(99)
    lens = np.array([len(r) for r in rs.reads], dtype=np.int64)
    start = np.where(rs.origin >= 0, rs.origin, (np.arange(rs.n) * 7) % (R - 400))
    delta = np.where(rng.random(rs.n) < 0.2, rng.integers(-3, 4, rs.n), 0) + np.where(rng.random(rs.n) < 0.05, rng.choice([-12, 12], rs.n), 0)
    wlen = np.clip(lens + delta, 0, R - start)
    return start.astype(np.uint32), wlen.astype(np.uint32)


def _sneaky(env, set_name, pres, stream):
    import torch

    rs = env.sets[set_name]
    p = presented(env, set_name, pres)
    rstart, rlen = _windows(rs, len(env.ref))
    out = ah.Out(rs.n, np.uint8, p.device)
    if p.device:
        ts, tl = torch.from_numpy(rstart.view(np.int32)).cuda(), torch.from_numpy(rlen.view(np.int32)).cuda()
        torch.cuda.synchronize()
        a, b = ts.data_ptr(), tl.data_ptr()
    else:
        a, b = rstart.ctypes.data, rlen.ctypes.data
    rc = env.lib.zsw_sneaky_snake_batch(env.h, p.ref(), a, b, C.c_float(THRESHOLD), out.ptr, ah.stream_ptr(stream))
    assert rc == 0, env.lib.zsw_last_error_string(env.h).decode()
    ah._sync(stream, p.device)
    assert out.guards_intact()
    res = out.data()
    assert not (res == ah.FILL).any()
    return res, rstart, rlen


SNEAKY = [(s, p, st) for s in FIXED_SETS for p in PRESENTATIONS[:4] for st in STREAMS] + \
         [("ragged", p, st) for p in ("device-ragged", "host-ragged") for st in STREAMS]


@pytest.mark.parametrize("set_name,pres,stream", SNEAKY, ids=["zsw_sneaky_snake_batch-" + "-".join(c) for c in SNEAKY])
def test_sneaky_snake_presentations(env, set_name, pres, stream):
    """no packed presentation: the filter compares raw bytes (test_gpu_filter.py has the misuse cases)"""
    rs, o = env.sets[set_name], env.oracle
    key = ("zsw_sneaky_snake_batch", set_name)
    if key not in env.base:
        res, rstart, rlen = _sneaky(env, set_name, base_pres(set_name), None)
        code = {False: 0, True: 1, None: 2}
        want = np.array(ah.pmap(lambda i: code[o.sneaky_snake(env.ref[rstart[i]:rstart[i] + rlen[i]], rs.reads[i], THRESHOLD)], range(rs.n)), dtype=np.uint8)
        bad = np.nonzero(res != want)[0]
        assert bad.size == 0, (bad[:5], res[bad[:5]], want[bad[:5]])
        assert set(want.tolist()) == {0, 1, 2}
        env.base[key] = res
    got, _, _ = _sneaky(env, set_name, pres, stream_of(env, stream))
    assert np.array_equal(got, env.base[key])


# ---- two contexts behind a group ---------------------------------------------------------------------------------------------

GROUP = [(g, s, p) for g in ("zsw_group_score_batch_from", "zsw_group_align_batch_from", "zsw_group_align_3pass_batch_from")
         for s in FIXED_SETS for p in ("host-fixed", "host-ragged", "host-packed4")] + \
        [(g, "ragged", "host-ragged") for g in ("zsw_group_score_batch_from", "zsw_group_align_batch_from", "zsw_group_align_3pass_batch_from")]


@pytest.fixture(scope="module")
def group(env):
    g = C.c_void_p()
    ids = (C.c_int * 2)(0, 0)
    assert env.lib.zsw_group_create(ids, 2, C.byref(g)) == 0
    w = np.ascontiguousarray(env.dna.signed_weights(), dtype=np.int8)
    im = np.ascontiguousarray(env.dna.mapping.index_map, dtype=np.uint8)
    r = np.frombuffer(env.ref, dtype=np.uint8)
    assert env.lib.zsw_group_set_scoring(g, w.ctypes.data, 5, im.ctypes.data, -10, -1) == 0
    assert env.lib.zsw_group_set_reference(g, r.ctypes.data, len(r)) == 0
    yield g
    env.lib.zsw_group_destroy(g)


@pytest.mark.parametrize("fn_name,set_name,pres", GROUP, ids=["-".join(c) for c in GROUP])
def test_group_presentations_equal_one_context(env, group, fn_name, set_name, pres):
    """two contexts on device 0, each with half the reads: the arrays of the single-context call, ciglets shard after shard"""
    single = ENTRY[fn_name.replace("_group", "")]
    want = baseline(env, single, set_name)
    p = presented(env, set_name, pres)
    n = p.rs.n
    fn = getattr(env.lib, fn_name)
    msg = lambda: env.lib.zsw_group_last_error_string(group).decode()
    o = {k: ah.Out(n, ah.DTYPES[k], False) for k in single.arrays()}
    if single.kind == "score":
        assert fn(group, p.ref(), 8, 256, o["score"].ptr, o["status"].ptr, o["tier"].ptr) == 0, msg()
    else:
        total = C.c_uint64(0)
        head = (group, p.ref(), 8, 256, single.invert, o["aln"].ptr, o["status"].ptr, o["tier"].ptr)
        assert fn(*head, None, None, 0, C.byref(total)) == -1 and "capacity" in msg()
        t = int(total.value)
        assert t == int(want["total"][0])
        o["inc"], o["op"] = ah.Out(t, np.uint32, False), ah.Out(t, np.uint8, False)
        assert fn(*head, o["inc"].ptr, o["op"].ptr, t - 1, C.byref(total)) == -1 and int(total.value) == t
        assert all(a.guards_intact() for a in o.values())
        assert fn(*head, o["inc"].ptr, o["op"].ptr, t, C.byref(total)) == 0, msg()
    got = {}
    for k, a in o.items():
        assert a.guards_intact(), k
        got[k] = a.data()
    assert not (got["status"] == ah.FILL).any()
    if single.kind == "align":
        got["total"] = np.array([total.value], dtype=np.uint64)
    ah.assert_same(got, want, f"{fn_name} {set_name} {pres}")


# ---- two asynchronous calls back to back on one stream -----------------------------------------------------------------------

PAIRS = [
    (("zsw_score_batch", "L150", "device-fixed"), ("zsw_score_ranges_batch", "L151", "device-fixed")),
    (("zsw_score_ranges_batch", "L150", "device-fixed"), ("zsw_score_shared_batch", "L151", "device-fixed")),
    (("zsw_score_batch", "ragged", "device-ragged"), ("zsw_score_ends_batch", "L151", "device-fixed")),
]


@pytest.mark.parametrize("first,second", PAIRS, ids=[f"{a[0]}-{a[1]}-then-{b[0]}-{b[1]}" for a, b in PAIRS])
def test_two_async_calls_on_one_stream(env, first, second):
    """Consecutive asynchronous calls on the same stream are ordered (include/zoe_sw.h): two device calls of different entry
    points, batches and output arrays, queued without a synchronisation between them, equal the calls made one at a time."""
    calls = [ah.Call(env._lib, env.lib, env.h, ENTRY[e], presented(env, s, p), env.own) for e, s, p in (first, second)]
    for c in calls:
        c.launch()  # no host synchronisation in between
    for c, (e, s, p) in zip(calls, (first, second)):
        ah.assert_same(c.collect(), baseline(env, ENTRY[e], s), f"{e} {s} queued back to back")
