"""The third pass of the 3-pass alignment (zsw_threepass.hip: threepass_kernel, zsw_capi.hip: threepass_third_pass) at the edges of
its decisions: the band limit, the band doublings, boxes of a few residues, MAXC ciglets, slots held at SLOT_CAP, rows that
exceed a slot, and more DP reads than slots.

The reads come from tests/threepass_edge_reads.py, whose CPU test proves with the oracle alone that each meets its condition.
Every batch runs through zsw_align_3pass_batch_from (and, for the groups where the roles matter, through
zsw_align_3pass_shared_batch_from, where the box's rows are the read's) as a device-ragged and a host-ragged batch, with
zsw_debug_threepass_records on. Asserted for EVERY read: status, tier, the alignment record and its ciglets against the oracle,
and the eight integers of the route record against the generator's replay of three_pass.rs and of the slot rule — so a read that
reaches the right CIGAR by the wrong route (a rerun it did not need, an attempt too many) fails. Each test then requires the
(route, attempts, launch, reason) tuples its group was built for among those observed.

Exact-fit and nearest-fit reads are repeated about 200 times through a batch of ordinary DP reads: a write past a slot's end lands
in a neighbouring block's interleaved region, which is then in use.

Out of scope: a bounding box beyond 2^31 bytes and soft clips beyond 2^24 bases cannot be reached at test size."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import abi_helpers as ah
import threepass_edge_reads as ter

pytestmark = pytest.mark.gpu

S_ = 0
UNSET = -7
PRESENTATIONS = ("device-ragged", "host-ragged")


@dataclass(frozen=True)
class Entry(ah.Entry):
    inv: int = 0

    @property
    def invert(self) -> int:
        return self.inv


def entry_of(role: str, invert: int) -> Entry:
    name = "zsw_align_3pass_batch_from" if role == "direct" else "zsw_align_3pass_shared_batch_from"
    return Entry(name, "align", True, role == "shared", True, invert)


class Env:
    pass


@pytest.fixture(scope="module")
def env(oracle):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib

    e = Env()
    e.za, e._lib, e.lib, e.oracle, e.torch = zoe_amd, _lib, _lib.load(), oracle, torch
    e.ctx = {}
    yield e
    for h in e.ctx.values():
        e.lib.zsw_destroy(h)


def context(env, g: ter.Group):
    """one context per group: its scheme, its reference as the reference and as the shared role's profile sequence"""
    if g.name not in env.ctx:
        ma, mi, go, ge = g.scheme
        m = env.za.WeightMatrix.new_dna_matrix(ma, mi, b"N")
        sc = ter.scoring(env.oracle, g.scheme)
        assert np.array_equal(m.signed_weights(), sc.weights) and np.array_equal(m.mapping.index_map, sc.index_map)
        env.ctx[g.name] = ah.new_context(env._lib, env.lib, m, go, ge, g.ref, pseq=g.ref)
    return env.ctx[g.name]


def run(env, g: ter.Group, role: str, pres: str, invert: int, reads):
    """one alignment call with the route records on -> (results, records int32[n, 8])"""
    h = context(env, g)
    n = len(reads)
    rs = ah.ReadSet(g.name, g.ref, list(reads), 0, np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64))
    rec = env.torch.full((n, 8), UNSET, dtype=env.torch.int32, device="cuda")
    env.torch.cuda.synchronize()
    assert env.lib.zsw_debug_threepass_records(h, C.c_void_p(rec.data_ptr())) == 0
    try:
        res = ah.Call(env._lib, env.lib, h, entry_of(role, invert), ah.Presented(env._lib, rs, pres)).run().collect()
        env.torch.cuda.synchronize()
    finally:
        assert env.lib.zsw_debug_threepass_records(h, None) == 0
    return res, rec.cpu().numpy()


def check(env, g: ter.Group, role: str, invert: int, reads, res, rec):
    """every read against the oracle and the replay; returns the (route, attempts, launch, reason) tuples observed"""
    exp = ter.expected(env.oracle, g, role)
    seen = set()
    for i, s in enumerate(reads):
        e = exp[s]
        got = ah.aln_key(res, i)
        got = got + (int(res["tier"][i]),) if got[0] == S_ else got
        assert got == e.keys[invert], (g.name, role, invert, i, got, e.keys[invert])
        if e.record is None:
            assert (rec[i] == UNSET).all(), (g.name, role, i, rec[i])  # no alignment: the record is left alone
            continue
        assert tuple(int(x) for x in rec[i]) == e.record, (g.name, role, invert, i, rec[i], e.record, e.replay.trace)
        seen.add(ter.edge(e.record))
    assert g.must[role] <= seen, (g.name, role, sorted(g.must[role] - seen))
    return seen


def run_group(env, name: str, inverts=None):
    g = ter.group(name)
    reads, _ = ter.batch_reads(g)
    for role in g.roles:
        for k, pres in enumerate(PRESENTATIONS):
            # the role's usual `invert` on the device batch, the other one on the host batch where the group asks for both
            usual = 1 if role == "shared" else 0
            for invert in (inverts or ((usual,) if k == 0 or len(g.inverts) == 1 else (1 - usual,))):
                res, rec = run(env, g, role, pres, invert, reads)
                check(env, g, role, invert, reads, res, rec)
    return g, reads


def test_band_limit(env):
    """band0 == max_band is one accepted attempt, band0 == max_band + 1 the scalar alignment without an attempt: deletions and
    insertions, both roles"""
    run_group(env, "band")


def test_band_doublings(env):
    """1 .. 6 attempts, accepted bands 1 .. 32, on equal-length boxes whose diagonal does not add up to the score"""
    run_group(env, "doubling")


def test_doubling_past_max_band(env):
    """three rejected attempts, the fourth band exceeds max_band: the scalar alignment"""
    run_group(env, "past")


def test_tiny_boxes_and_diag_sum(env):
    """boxes of 2 .. 5 query residues through the DP (max_band 0, 1, 1, 2) and shortcut boxes of 1, 2, 3, 4, 5, 7, 8 residues, one
    on the reference's last base: the word loop of diag_sum and its tail"""
    run_group(env, "tiny")


def test_ciglets_at_maxc(env):
    """MAXC ciglets stay in the first launch, one more goes to the rerun (reason 4) — with both `invert` values on both
    presentations, since n_ciglets is counted differently there and the decision is not"""
    run_group(env, "ciglets", inverts=(0, 1))


def test_slots_at_the_cap(env):
    """With the first launch's slot held at SLOT_CAP: scalar boxes that fill it to the byte stay, one row more goes to the rerun
    (reason 3); banded attempts two and three bytes short of it stay, two and four bytes over go (reason 2, with the band) — first
    attempts and doubled ones. About 200 copies of each among 2400 short DP reads."""
    g, reads = run_group(env, "cap")
    assert len(reads) > 4000


@pytest.mark.parametrize("q, d", ter.FILLS)
def test_banded_attempt_fills_an_uncapped_slot(env, q, d):
    """band = max_band on an odd query range: the attempt needs what the box needs, and the box sets the slot, a multiple of 64:
    the attempt fills the slot to the byte and stays — a deletion and an insertion, 70 copies each among short banded reads"""
    run_group(env, f"fill{q}")


def test_rows_alone_exceed_the_slot(env):
    """the shortest read whose two DP rows alone exceed SLOT_CAP: reason 1, finished by the rerun; one base less and the rows are
    the slot to the byte: the read stays for the band loop, whose first attempt does not fit (reason 2)"""
    run_group(env, "rows")


def test_more_dp_reads_than_slots(env):
    """slots + 200 DP reads at the capped slot size: a thread walks a second read through a slot that holds the first one's rows
    and flag bytes. Every read against the oracle; a second call on the same context gives identical results and records."""
    g = ter.group("reuse")
    c = ter.constants()
    reads, _ = ter.batch_reads(g)
    assert len(reads) == ter.slot_count(c["SLOT_CAP"], 1 << 30, c) + ter.REUSE_EXTRA + 1
    first = None
    for pres in PRESENTATIONS:
        for _ in range(2 if pres == PRESENTATIONS[0] else 1):
            res, rec = run(env, g, "direct", pres, 0, reads)
            check(env, g, "direct", 0, reads, res, rec)
            if first is None:
                first = (res, rec)
            else:
                ah.assert_same(res, first[0], f"reuse, {pres}")
                assert np.array_equal(rec, first[1])
