"""The reads of tests/threepass_edge_reads.py meet the conditions they were built for — checked against the oracle alone, through
the generator's replay of three_pass.rs, so that the GPU tests built on them (tests/test_gpu_threepass_edges.py) cannot pass
because a read missed its edge."""
import numpy as np
import pytest

import threepass_edge_reads as ter

S_ = 0


def _check_cases(oracle, name):
    """every case's replayed record is the designed one (direct role), and every role's batch shows the tuples it must"""
    g = ter.group(name)
    for role in g.roles:
        exp = ter.expected(oracle, g, role)
        seen = set()
        for e in exp.values():
            if e.record is not None:
                seen.add(ter.edge(e.record))
        for cs in g.cases:
            e = exp[cs.seq]
            print(f"{name} {role} {cs.tag}: box {e.replay.rlen} x {e.replay.qlen}, attempts {e.replay.trace}, record {e.record}")
            assert e.replay.status == S_, (name, role, cs.tag)
            if cs.want is not None and role == "direct":
                assert e.record[:6] == cs.want, (name, cs.tag, e.record, cs.want)
        assert g.must[role] <= seen, (name, role, sorted(g.must[role] - seen))
    return g


def test_constants_and_slot_arithmetic():
    c = ter.constants()
    assert c["SLOT_CAP"] % 64 == 0 and c["MAXC"] >= 2 and c["BUDGET"] > c["SLOT_CAP"] and c["MAX_SLOTS"] % 64 == 0
    assert ter.rows_bytes(1) == 48 and ter.rows_bytes(2) == 48 and ter.rows_bytes(3) == 64 and ter.slot_need(3, 2) == 54
    # more DP reads than slots: the count at the cap is what the budget gives, a multiple of the block's 64 lanes
    slots = ter.slot_count(c["SLOT_CAP"], 1 << 30, c)
    assert slots == min(c["BUDGET"] // c["SLOT_CAP"], c["MAX_SLOTS"]) // 64 * 64 and ter.slot_count(c["SLOT_CAP"], 65, c) == 128
    assert ter.slot_count(1 << 31, 1000, c) == 64 and ter.slot_count(64, 1 << 30, c) == c["MAX_SLOTS"]


def test_band_limit(oracle):
    g = _check_cases(oracle, "band")
    exp = ter.expected(oracle, g, "direct")
    for cs in g.cases:
        r = exp[cs.seq].replay
        d = int(cs.tag.split("d")[-1])
        assert abs(r.rlen - r.qlen) == d and (r.qlen - 1) // 2 == 20 and (r.qlen > r.rlen) == cs.tag.startswith("ins"), (cs.tag, r)
        assert [b for b, _, _ in r.trace] == ([20] if d == 19 else [])


def test_doublings(oracle):
    g = _check_cases(oracle, "doubling")
    for role in g.roles:
        exp = ter.expected(oracle, g, role)
        for k, cs in enumerate(g.cases):
            r = exp[cs.seq].replay
            assert r.rlen == r.qlen and not r.shortcut  # the equal-length box whose diagonal does not add up to the score
            assert [(b, ok) for b, ok, _ in r.trace] == [(1 << j, j == k) for j in range(k + 1)], (role, cs.tag, r.trace)


def test_doubling_past_max_band(oracle):
    g = _check_cases(oracle, "past")
    for role in g.roles:
        r = ter.expected(oracle, g, role)[g.cases[0].seq].replay
        bands = [b for b, _, _ in r.trace]
        assert len(bands) >= 2 and not any(ok for _, ok, _ in r.trace) and bands[-1] <= (r.qlen - 1) // 2 < 2 * bands[-1], (role, r)


def test_ciglets(oracle):
    g = _check_cases(oracle, "ciglets")
    maxc = ter.constants()["MAXC"]
    for role in g.roles:
        exp = ter.expected(oracle, g, role)
        stays, goes = (exp[cs.seq] for cs in g.cases)
        assert stays.replay.ncig == maxc and goes.replay.ncig > maxc, (role, stays.replay.ncig, goes.replay.ncig)
        assert stays.record[3:5] == (1, 0) and goes.record[3:5] == (2, 4)
        for e in (stays, goes):  # n_ciglets of the inverted alignment is counted otherwise; the decision is not
            assert e.keys[0][0] == e.keys[1][0] == S_ and e.keys[0][4] != e.keys[1][4]
            assert e.keys[0][4].count("D" if role == "direct" else "I") in (15, 16)


def test_tiny_boxes(oracle):
    g = _check_cases(oracle, "tiny")
    want_q = {"direct": {2, 3, 4, 5}, "shared": {4, 5}}  # no DP box of one query residue exists among the reads enumerated
    for role in g.roles:
        exp = ter.expected(oracle, g, role)
        dp = {}
        for cs in g.cases:
            r = exp[cs.seq].replay
            if cs.want is not None:
                k = len(cs.seq)
                assert r.shortcut and r.rlen == r.qlen == k, (role, cs.tag, r)
                if role == "direct":
                    assert r.qr == (0, k)  # ends on the read's last base
            elif r.status == S_ and not r.shortcut:
                dp.setdefault(r.qlen, []).append(r)
        assert want_q[role] <= set(dp), (role, sorted(dp))
        assert all((q - 1) // 2 == mb for q, mb in zip((1, 2, 3, 4, 5), (0, 0, 1, 1, 2)))
        if role == "shared":  # a banded attempt at max_band = 2
            assert any(r.route == 2 for r in dp[5])
        last = exp[b"TG"].replay
        assert (last.rr if role == "direct" else last.qr)[1] == len(g.ref)  # ends on the reference's last base
    assert sorted({len(s) for s in ter.TINY_SHORTCUT}) == [1, 2, 3, 4, 5, 7, 8]


def test_slots_at_the_cap(oracle):
    g = _check_cases(oracle, "cap")
    c = ter.constants()
    cap = c["SLOT_CAP"]
    exp = ter.expected(oracle, g, "direct")
    by = {cs.tag.rsplit(" ", 1)[0]: [] for cs in g.cases}
    for cs in g.cases:
        by[cs.tag.rsplit(" ", 1)[0]].append(exp[cs.seq])
    (st,) = by["setter"]
    assert ter.slot_need(st.replay.rlen, st.replay.qlen) >= cap and st.record[6] == cap
    for e in by["scalar fits"]:
        assert ter.slot_need(e.replay.rlen, e.replay.qlen) == cap and e.replay.trace == ()
    for e in by["scalar over"]:
        assert ter.slot_need(e.replay.rlen, e.replay.qlen) == cap + e.replay.qlen and e.record[6] > cap
    for kind, attempts in (("banded", 1), ("doubled", 2)):
        (fits,), (over,) = by[f"{kind} fits"], by[f"{kind} over"]
        for e, sign in ((fits, -1), (over, 1)):
            r = e.replay
            band = r.trace[-1][0]
            assert len(r.trace) == attempts and r.trace[-1][1] and not any(ok for _, ok, _ in r.trace[:-1])
            dist = ter.rows_bytes(r.qlen) + r.rlen * (2 * band + 1) - cap
            print(kind, "fits" if sign < 0 else "over", "distance to the slot", dist, "of a band row of", 2 * band + 1)
            assert (dist <= 0 if sign < 0 else dist > 0) and abs(dist) < 2 * band + 1
        assert over.record[4:6] == (2, over.replay.trace[-1][0])
        if attempts == 2:  # the smaller band fits, and is rejected
            r = over.replay
            assert ter.rows_bytes(r.qlen) + r.rlen * (2 * r.trace[0][0] + 1) <= cap
    assert sum(cs.copies for cs in g.cases) > 10 * ter.CAP_COPIES and len(g.filler) > 2000


@pytest.mark.parametrize("q, d", ter.FILLS)
def test_banded_attempt_fills_an_uncapped_slot(oracle, q, d):
    g = _check_cases(oracle, f"fill{q}")
    exp = ter.expected(oracle, g, "direct")
    e = exp[g.cases[0].seq]
    r = e.replay
    band = r.trace[0][0]
    assert (r.qlen, r.rlen) == (q, q + d) and r.trace == ((band, True, S_),) and band == (q - 1) // 2
    assert ter.rows_bytes(q) + r.rlen * (2 * band + 1) == e.record[6] < ter.constants()["SLOT_CAP"]
    assert all(x.record[6] == e.record[6] and x.record[0] == 2 for x in exp.values())


def test_rows_alone(oracle):
    g = _check_cases(oracle, "rows")
    cap = ter.constants()["SLOT_CAP"]
    over, fills = (ter.expected(oracle, g, "direct")[cs.seq] for cs in g.cases)
    r = over.replay
    assert ter.rows_bytes(r.qlen) > cap == ter.rows_bytes(r.qlen - 1) and r.qlen == len(g.cases[0].seq)
    assert fills.replay.qlen == r.qlen - 1 and over.record[4] == 1 and fills.record[4:6] == (2, 1)


def test_slot_reuse(oracle):
    g = _check_cases(oracle, "reuse")
    c = ter.constants()
    exp = ter.expected(oracle, g, "direct")
    slots = ter.slot_count(c["SLOT_CAP"], 1 << 30, c)
    reads, _ = ter.batch_reads(g)
    dp = sum(1 for s in reads if exp[s].record is not None and exp[s].record[0] != 1)
    assert dp == len(reads) == slots + ter.REUSE_EXTRA + 1 and len(exp) == ter.REUSE_POOL + 1, (dp, slots, len(exp))
    assert all(e.record is None or e.record[3] < 2 for e in exp.values())  # nobody needs the rerun: both walks share one launch
    assert {e.record[6] for e in exp.values() if e.record is not None and e.record[0] != 1} == {c["SLOT_CAP"]}
    bands = {e.record[1] for e in exp.values() if e.record is not None and e.record[0] == 2}
    assert len(bands) >= 4, bands


def test_unbanded_search_is_recorded(oracle):
    """An attempt that reproduces the score while its traceback leaves the band: what the search on the CPU gave."""
    for scheme, ref, read in ter.UNBANDED:
        r = ter.replay(oracle, ter.scoring(oracle, scheme), read, ref)
        assert any(st != S_ for _, _, st in r.trace), (scheme, ref, read)
    assert ter.UNBANDED or ter.UNBANDED_TRIED >= 100000
    if not ter.UNBANDED:  # the search as it was run, for a few reads: a hit here is a read to add
        assert ter.search_unbanded(oracle, ter.SCHEME_TINY, 200, seed=7) is None
