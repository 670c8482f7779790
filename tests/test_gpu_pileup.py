"""GPU tests of zsw_pileup_batch and zsw_consensus_from_counts through the C ABI: the device against tests/pileup_ref.py on every bin
of every site and every insertion entry.

Shapes are the smallest at which the kernels can go wrong (G = 64 lanes per alignment, 8 alignments per block, accumulators in LDS
up to LDS_SITES sites): column runs around G and 2G, runs that start at 0 and end on the last position, every op, reads and a
context sequence with lower-case, U, IUPAC and invalid bytes, records of 0 / 1 / G / G + 1 / 70 ciglets, 5,000 identical reads on
one place, accumulating calls, ZSW_PILEUP_CLEAR, a pre-filled table with guard entries, sequences on both sides of the LDS
threshold, batches of one block +- 1 read, of a few thousand and of none, fixed / ragged / host presentations; then the records of
the alignment entry points of both roles and both `invert` values end to end with the identities against zsw_annotate_batch, the
hand-built malformed records of tests/test_annotate_model.py (clean under the sanitizers in tests/test_pileup_model.py first), the
consensus with its known answers and ties, a refinement round that stays on the card, the argument errors and the Python layer."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import abi_helpers as ah
import annotate_ref as ar
import pileup_ref as pr
from test_gpu_annotate import Annotate, Records, align, built_items, make_seq, place, read_set, rec, records_of

pytestmark = pytest.mark.gpu

G, BLOCK_READS, LDS_SITES = 64, 8, 4096  # zsw_pileup.hpp: PILEUP_G, PILEUP_WAVES, PILEUP_LDS_SITES_MAX
GO, GE = -10, -1
COUNTS_DT = np.dtype([("bin", "<u4", (8,))])              # zsw_site_counts
INS_DT = np.dtype([("runs", "<u4"), ("bases", "<u4")])    # zsw_site_insertions
PATTERN = 0xA5A5A5A5                                       # ah.FILL in every byte: what a guarded array holds before the call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib

    lib = _lib.load()
    m = zoe_amd.WeightMatrix.new(zoe_amd.DNA_PROFILE_MAP, 2, -5, b"N")
    return {"za": zoe_amd, "_lib": _lib, "lib": lib, "m": m, "w": m.signed_weights(), "im": np.asarray(m.mapping.index_map, dtype=np.uint8)}


def test_the_constants_the_shapes_are_built_from(env):
    hpp = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_pileup.hpp")).read()
    assert int(re.search(r"PILEUP_G = (\d+);", hpp).group(1)) == G and int(re.search(r"PILEUP_WAVES = (\d+);", hpp).group(1)) == BLOCK_READS
    assert int(re.search(r"PILEUP_LDS_SITES_MAX = (\d+);", hpp).group(1)) == LDS_SITES
    assert ah.FILL * 0x01010101 == PATTERN


# ---- one call ------------------------------------------------------------------------------------------------------------------

class Pileup:
    """zsw_pileup_batch calls on a presented batch; the tables in guarded arrays that hold PATTERN in every counter before the first"""

    def __init__(self, env, h, p: ah.Presented, seq_len: int, r: Records, with_ins: bool = True, stream=None):
        self.env, self.h, self.p, self.L, self.r, self.stream = env, h, p, seq_len, r, stream
        self.arrays = [place(a, p.device) for a in (r.aln, r.status, r.inc, r.op)]
        self.counts = ah.Out(seq_len, COUNTS_DT, p.device)
        self.ins = ah.Out(seq_len + 1, INS_DT, p.device) if with_ins else None
        self.n_bad = C.c_uint64(12345)

    def call(self, flags, p=None, arrays=None, n_ciglets=None):
        p, a = p or self.p, arrays or self.arrays
        return self.env["lib"].zsw_pileup_batch(self.h, p.ref(), flags, a[0][0], a[1][0], a[2][0], a[3][0], len(self.r.inc) if n_ciglets is None else n_ciglets,
                                                self.counts.ptr, self.ins.ptr if self.ins else None, C.byref(self.n_bad), ah.stream_ptr(self.stream))

    def msg(self):
        return self.env["lib"].zsw_last_error_string(self.h).decode()

    def tables(self, base=PATTERN):
        """(counts (L, 8), ins (L + 1, 2)) with `base` taken off every counter, modulo 2^32; the guards checked"""
        import torch

        torch.cuda.synchronize()
        assert self.counts.guards_intact() and (self.ins is None or self.ins.guards_intact()), "guard entries were written"
        c = self.counts.data()["bin"].reshape(self.L, 8) - np.uint32(base)
        i = None
        if self.ins is not None:
            d = self.ins.data()
            i = np.stack([d["runs"], d["bases"]], axis=1) - np.uint32(base)
        return c, i

    def run(self, flags, base=PATTERN):
        assert self.call(flags) == 0, self.msg()
        return self.tables(base) + (int(self.n_bad.value),)


def expect(rs: ah.ReadSet, seq: bytes, flags: int, r: Records):
    return pr.pileup(r.aln, r.status, r.inc, r.op, rs.reads, seq, flags)


def same(got, want, what):
    assert got[2] == want[2], (what, "n_bad", got[2], want[2])
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), f"{what}: {len(bad)} counters differ, first (site, bin) {bad[:4].tolist()}: got {got[0][bad[0][0]]}, want {want[0][bad[0][0]]}"
    if got[1] is not None:
        bad = np.argwhere(got[1] != want[1])
        assert not len(bad), f"{what}: {len(bad)} insertion entries differ, first {bad[:4].tolist()}: got {got[1][bad[0][0]]}, want {want[1][bad[0][0]]}"


# ---- built shapes ----------------------------------------------------------------------------------------------------------------

def dirty_seq(n, seed):
    """a sequence with lower case, U, N, IUPAC letters, a gap and invalid bytes among its bases"""
    rng = np.random.default_rng(seed)
    s = bytearray(make_seq(n, seed))
    alpha = b"acgtuUNnRYswKM.-#@"
    for k in rng.integers(0, n, max(4, n // 12)):
        s[k] = alpha[int(rng.integers(0, len(alpha)))]
    return bytes(s)


def extra_items(seq: bytes):
    """(read, status, record, ciglets), flags 0: what built_items (the annotate shapes) does not have"""
    R = len(seq)
    out = []

    def add(read, r, cigar, st=0):
        out.append((bytes(read), st, r, ar.parse_cigar(cigar)))

    other = bytes.maketrans(b"ACGTacgtUuNn", b"CGTAcgtaAaCc")
    for run in (1, G - 1, G, G + 1, 2 * G + 1):
        for s in (0, 11, R - run):                                   # a run that starts at 0, one that ends on the last position
            piece = seq[s:s + run]
            add(piece, rec((s, s + run), (0, run), R, run), f"{run}M")                                            # every column as expected
            add(piece.translate(other), rec((s, s + run), (0, run), R, run), f"{run}M")                           # every column a miss
            add(bytes(b if k & 1 else piece.translate(other)[k] for k, b in enumerate(piece)), rec((s, s + run), (0, run), R, run), f"{run}X")
            add(piece.swapcase().replace(b"t", b"u").replace(b"T", b"U"), rec((s, s + run), (0, run), R, run), f"{run}=")  # the other case, U for T
    add(b"RYSWKMBDHVryswkmbdhv.-#@\x00\xff" + seq[26:100], rec((0, 100), (0, 100), R, 100), "100M")
    add(seq[:10], rec((0, R), (0, 10), R, 10), f"10M{R - 10}D")                                                   # a gap range up to len
    add(seq[R - 10:], rec((0, R), (0, 10), R, 10), f"{R - 10}N10M")                                               # an N range from 0
    add(b"TT" + seq[:98], rec((0, 98), (0, 100), R, 100), "2I98M")                                                # an insertion in front of 0
    add(seq[R - 98:] + b"TT", rec((R - 98, R), (0, 100), R, 100), "98M2I")                                        # ... and in front of len
    add(seq[20:70] + b"GGT" + seq[70:117], rec((20, 117), (0, 100), R, 100), "50M2I1I47M")                        # two runs in one place
    add(seq[20:30] + b"TTTTT" + seq[35:120], rec((20, 120), (0, 100), R, 100), "5H2P10M5N5S85M3H")
    add(seq[20:70] + seq[75:125], rec((20, 125), (0, 100), R, 100), "50M5D50M")
    return out


def swap_items(seq: bytes):
    """READ_IS_REF: the record's reference is the read, its query seq"""
    R = len(seq)
    out = []

    def add(read, rr, qr, cigar, st=0):
        out.append((bytes(read), st, rec(rr, qr, len(read), R), ar.parse_cigar(cigar)))

    clip = lambda n: f"{n}S" if n else ""
    for s, L in ((0, 150), (R - 150, 150), (R - 1, 1), (33, G), (33, G + 1), (R - 129, 129)):
        read = bytearray(seq[s:s + L])
        read[L // 2] = ord("n")
        add(read, (0, L), (s, s + L), f"{clip(s)}{L}M{clip(R - s - L)}")
    add(seq[20:70] + seq[75:120], (0, 95), (20, 120), f"20S50M5I45M{R - 120}S")            # I: positions of seq opposite nothing
    add(seq[20:70] + b"GGG" + seq[70:120], (0, 103), (20, 120), f"20S50M3D50M{R - 120}S")  # D: read bases opposite nothing
    add(seq[20:70] + b"GGG" + seq[70:120], (0, 103), (20, 120), f"20S50M3N50M{R - 120}S")  # N: nothing
    add(b"GG" + seq[20:120], (2, 102), (20, 120), f"20S100M{R - 120}S")                    # ref_start into the read
    add(seq[R - 5:] + b"T", (0, 6), (R - 5, R), f"{R - 5}S5M1D")                           # an insertion in front of len
    add(seq[20:120], (0, 100), (20, 120), f"20S101M{R - 121}S")                            # leaves the read: counted in n_bad
    return out


def run_items(env, seq, items, pres, fixed_len=0, flags=0, with_ins=True):
    _lib, lib = env["_lib"], env["lib"]
    h = ah.new_context(_lib, lib, env["m"], GO, GE, seq)
    try:
        rs = read_set("built", seq, [it[0] for it in items], fixed_len)
        r = records_of([it[1:] for it in items])
        want = expect(rs, seq, flags, r)
        for p in pres:
            got = Pileup(env, h, ah.Presented(_lib, rs, p), len(seq), r, with_ins).run(flags)
            same(got, want, f"{p} n={rs.n}")
        return want
    finally:
        lib.zsw_destroy(h)


def test_built_shapes_ragged_and_host(env):
    seq = dirty_seq(700, 5)
    items = built_items(seq) + extra_items(seq)
    counts, ins, bad = run_items(env, seq, items, ("device-ragged", "host-ragged"))
    assert bad == 0 and ins[0].tolist() == [1, 2] and ins[700].tolist() == [1, 2] and ins[70, 0] >= 2
    assert all(counts[:, b].sum() > 0 for b in range(8)) and max(len(it[3]) for it in items) >= 70
    run_items(env, seq, items, ("device-ragged",), with_ins=False)


def test_built_shapes_fixed(env):
    seq = dirty_seq(420, 6)
    run_items(env, seq, built_items(seq, 150), ("device-fixed", "host-fixed", "device-ragged"), fixed_len=150)


def test_the_role_swap(env):
    seq = dirty_seq(700, 7)
    counts, ins, bad = run_items(env, seq, swap_items(seq), ("device-ragged", "host-ragged"), flags=pr.READ_IS_REF)
    assert bad == 1 and counts[:, pr.GAP].sum() >= 5 and ins[70].tolist() == [1, 3] and ins[700].tolist() == [1, 1]


@pytest.mark.parametrize("n", [0, 1, BLOCK_READS - 1, BLOCK_READS, BLOCK_READS + 1, 3000])
def test_batch_sizes(env, n):
    seq = dirty_seq(700, 8)
    items = built_items(seq) + extra_items(seq)
    items = [items[(k * 7) % len(items)] for k in range(n)]
    counts, _, _ = run_items(env, seq, items, ("device-ragged",) if n else ("device-ragged", "host-ragged"))
    assert counts.any() == (n > 0)  # an empty batch is ZSW_OK and leaves the pre-filled table as it was


@pytest.mark.parametrize("R", [LDS_SITES, LDS_SITES + 1])
def test_both_sides_of_the_lds_threshold(env, R):
    """a sequence whose accumulators a block keeps in LDS, and one that is one site too long, where every add goes to the global
    workspace: reads cut from its first and its last bases, ranges that end on the last position (entry `len` of the difference
    arrays), in both roles"""
    seq = dirty_seq(R, 9)
    items = [it for it in extra_items(seq)]
    for s, L in ((0, 150), (R - 150, 150), (R - 65, 65), (R - 1, 1), (LDS_SITES - 100, 100), (R // 2, 401)):
        read = bytearray(seq[s:s + L])
        read[L // 2] = ord("n")
        items.append((bytes(read), 0, rec((s, s + L), (0, L), R, L), ar.parse_cigar(f"{L}M")))
    items = [items[k % len(items)] for k in range(3 * len(items))]  # more than one block
    counts, ins, bad = run_items(env, seq, items, ("device-ragged", "host-ragged"))
    assert bad == 0 and counts[R - 1].sum() >= 9 and ins[R].tolist() == [3, 6]
    run_items(env, seq, swap_items(seq), ("device-ragged",), flags=pr.READ_IS_REF)


# ---- contention, accumulation, CLEAR, the pre-filled table --------------------------------------------------------------------------

def test_contention_accumulation_and_clear(env):
    """5,000 identical reads on one place: every touched counter is exactly 5,000 times one read's. The same batch over two
    accumulating calls gives the same table; ZSW_PILEUP_CLEAR forgets the pattern the table held; without it the pattern stays
    under the counts (Pileup.tables takes it off) and the guard entries are intact."""
    _lib, lib = env["_lib"], env["lib"]
    seq = dirty_seq(600, 10)
    read = bytearray(seq[100:150] + b"GT" + seq[150:180] + seq[185:200] + seq[210:255])
    for k in (0, 7, 63, 64, 65, len(read) - 1):
        read[k] = ord("n")
    item = (bytes(read), 0, rec((100, 255), (0, len(read)), 600, len(read)), ar.parse_cigar("50M2I30M5D15M10N45M"))
    one = expect(read_set("one", seq, [item[0]]), seq, 0, records_of([item[1:]]))
    assert one[2] == 0 and one[0].sum() == 155 and one[1].sum() == 3
    N = 5000
    rs = read_set("same", seq, [item[0]] * N, len(read))
    r = records_of([item[1:]] * N)
    h = ah.new_context(_lib, lib, env["m"], GO, GE, seq)
    try:
        for pres in ("device-fixed", "host-fixed"):
            p = Pileup(env, h, ah.Presented(_lib, rs, pres), 600, r)
            got = p.run(0)
            assert np.array_equal(got[0], one[0] * np.uint32(N)) and np.array_equal(got[1], one[1] * np.uint32(N)) and got[2] == 0, pres
            got = p.run(0)                                                   # a second call adds to the first
            assert np.array_equal(got[0], one[0] * np.uint32(2 * N)) and np.array_equal(got[1], one[1] * np.uint32(2 * N))
            got = p.run(pr.CLEAR, base=0)                                    # the pattern and both calls are forgotten
            assert np.array_equal(got[0], one[0] * np.uint32(N)) and np.array_equal(got[1], one[1] * np.uint32(N))
        half = N // 2
        halves = [(read_set("half", seq, [item[0]] * k, len(read)), records_of([item[1:]] * k)) for k in (half, N - half)]
        p = Pileup(env, h, ah.Presented(_lib, halves[0][0], "device-fixed"), 600, halves[0][1])
        assert p.call(0) == 0, p.msg()
        p2 = ah.Presented(_lib, halves[1][0], "device-fixed")
        assert p.call(0, p=p2, arrays=[place(a, True) for a in (halves[1][1].aln, halves[1][1].status, halves[1][1].inc, halves[1][1].op)],
                      n_ciglets=len(halves[1][1].inc)) == 0, p.msg()
        got = p.tables()
        assert np.array_equal(got[0], one[0] * np.uint32(N)) and np.array_equal(got[1], one[1] * np.uint32(N))
        empty = ah.Presented(_lib, read_set("none", seq, [], len(read)), "device-fixed")
        assert p.call(pr.CLEAR, p=empty) == 0                                # an empty batch with CLEAR zeroes the tables
        got = p.tables(base=0)
        assert not got[0].any() and not got[1].any()
    finally:
        lib.zsw_destroy(h)


# ---- end to end ------------------------------------------------------------------------------------------------------------------

ENTRY_POINTS = ("zsw_align_batch_from", "zsw_align_3pass_batch_from", "zsw_align_3pass_strands_batch_from", "zsw_align_shared_batch_from",
                "zsw_align_3pass_shared_batch_from")


@pytest.fixture(scope="module")
def mixed(env):
    """a few thousand synthetic reads of 150 bases and the mixed classes of the ABI tests (indels, ties, odd bytes, all-N, empty)"""
    from zoe_amd import synth

    ref_arr = synth.reference_host(2000)
    ref = bytes(ref_arr)
    rs = ah.mixed_set("pileup-mixed", ref, 220, 0, 20261020)
    # (a `-` byte of a read falls in the gap bin, which the identities of test_end_to_end give to the deleted bases alone: `.` instead)
    reads = [r.tobytes() for r in synth.reads_host(ref_arr, 777, 2200, 150)] + [r.replace(b"-", b".") for r in rs.reads]
    return read_set("pileup-e2e", ref, reads)


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_end_to_end(env, mixed, name, invert):
    """the records of every alignment entry point: device pile-up == pileup_ref on every bin and insertion entry; and against the
    stats zsw_annotate_batch gives for the same records: the bins but the gap bin sum to matches + mismatches, the gap bin to
    del_bases (ins_bases under the swap), the insertion bases to the other of the two, the runs likewise"""
    import torch

    _lib, lib = env["_lib"], env["lib"]
    shared = "shared" in name
    h = ah.new_context(_lib, lib, env["m"], GO, GE, None if shared else mixed.ref, mixed.ref if shared else None)
    try:
        rs = mixed
        if "strands" in name:  # a third of the reads from the other strand
            rc = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
            rs = read_set("mixed-both-strands", mixed.ref, [r.translate(rc)[::-1] if k % 3 == 0 else r for k, r in enumerate(mixed.reads)])
        p = ah.Presented(_lib, rs, "device-ragged")
        r, strand = align(env, h, name, p, invert)
        if strand is not None:  # pile up the batch as aligned: zsw_orient_batch
            assert strand.any() and not strand.all()
            st, tst = place(strand, True)
            out = torch.empty_like(p.keep[0])
            assert lib.zsw_orient_batch(h, p.ref(), st, out.data_ptr(), None) == 0
            torch.cuda.synchronize()
            flat, off = out.cpu().numpy(), rs.offsets
            rs = read_set("oriented", mixed.ref, [flat[int(off[i]):int(off[i + 1])].tobytes() for i in range(rs.n)])
            p = ah.Presented(_lib, rs, "device-ragged")
        flags = (ar.SHARED | (0 if invert else ar.READ_IS_REF)) if shared else (ar.READ_IS_REF if invert else 0)
        some = r.status == ah.S_
        assert some.sum() > 2000
        got = Pileup(env, h, p, len(mixed.ref), r).run(flags)
        same(got, expect(rs, mixed.ref, flags, r), f"{name} invert={invert}")
        counts, ins, bad = got
        assert bad == 0
        s = Annotate(env, h, p, flags, r, verbose=False).run()["stats"]
        swap = bool(flags & ar.READ_IS_REF)
        gap_field, ins_field = ("ins", "del") if swap else ("del", "ins")
        c64 = counts.astype(np.int64)
        assert c64.sum() - c64[:, pr.GAP].sum() == int(s["matches"].astype(np.int64).sum() + s["mismatches"].sum())
        assert c64[:, pr.GAP].sum() == int(s[gap_field + "_bases"].astype(np.int64).sum())
        assert int(ins[:, 1].astype(np.int64).sum()) == int(s[ins_field + "_bases"].astype(np.int64).sum())
        assert int(ins[:, 0].astype(np.int64).sum()) == int(s[ins_field + "_runs"].astype(np.int64).sum())
        assert c64[:, pr.GAP].sum() > 0 and ins.any()
    finally:
        lib.zsw_destroy(h)


# ---- malformed records -----------------------------------------------------------------------------------------------------------

def test_malformed_records_are_a_count(env):
    """the hand-built records of tests/test_annotate_model.py (clean under address and undefined-behaviour sanitizers through the same
    header in tests/test_pileup_model.py) in one batch, good reads between them: out_n_bad is their number, and the table is
    pileup_ref's over the good ones alone"""
    from test_annotate_model import READ, SEQ, status_cases

    _lib, lib = env["_lib"], env["lib"]
    cases = [(w, c) for w, c in status_cases() if c["flags"] == 0]
    # every case brings the whole ciglet arrays of its own call; in one call they follow each other, and the record whose ciglets
    # pass the end of its arrays goes last, so that they pass the end of these
    past = [k for k, (_, c) in enumerate(cases) if c["rec"]["ciglet_offset"] + c["rec"]["n_ciglets"] > len(c["inc"]) and c["rec"]["ciglet_offset"] < 2 ** 32]
    assert len(past) == 1
    cases.append(cases.pop(past[0]))
    reads, counted = [], []
    aln = np.zeros(2 * len(cases), dtype=ah.ALN_DTYPE)
    status, inc, op = [], [], []
    for k, (w, c) in enumerate(cases):
        i = len(reads)
        reads.append(c["read"])
        for f, v in c["rec"].items():
            aln[i][f] = v % 2 ** 64 if f == "ciglet_offset" else v
        if c["rec"]["ciglet_offset"] < 2 ** 32:
            aln[i]["ciglet_offset"] = c["rec"]["ciglet_offset"] + len(inc)
        status.append(c["status"])
        inc += c["inc"]
        op += c["op"]
        merged_h = ar.cigar_string(zip(c["inc"], c["op"])).startswith("4294967295H")  # a merge overflow of the verbose CIGAR: nothing is merged here
        counted.append(w in ar.ANNOTATED or merged_h)
        if k + 1 < len(cases):  # (nothing behind the last case: its ciglets must pass the end)
            i = len(reads)
            reads.append(READ)
            for f, v in rec((20, 120), (0, 100), len(SEQ), len(READ), 200).items():
                aln[i][f] = v
            aln[i]["n_ciglets"], aln[i]["ciglet_offset"] = 1, len(inc)
            status.append(0)
            inc.append(100)
            op.append(ord("M"))
            counted.append(True)
    n = len(reads)
    r = Records(aln[:n], status, inc, op)
    rs = read_set("malformed", SEQ, reads)
    n_bad = sum(1 for ok, st in zip(counted, status) if not ok and st == 0)
    assert n_bad >= 20
    keep = [k for k in range(n) if counted[k]]
    good = Records(r.aln[keep], r.status[keep], r.inc, r.op)
    want_good = pr.pileup(good.aln, good.status, good.inc, good.op, [reads[k] for k in keep], SEQ, 0)
    assert want_good[2] == 0
    h = ah.new_context(_lib, lib, env["m"], GO, GE, SEQ)
    try:
        for pres in ("device-ragged", "host-ragged"):
            got = Pileup(env, h, ah.Presented(_lib, rs, pres), len(SEQ), r).run(0)
            same(got, expect(rs, SEQ, 0, r), "malformed " + pres)
            assert got[2] == n_bad and np.array_equal(got[0], want_good[0]) and np.array_equal(got[1], want_good[1])
    finally:
        lib.zsw_destroy(h)


# ---- consensus -------------------------------------------------------------------------------------------------------------------

def consensus(env, h, rows, flags=0, fallback=None, device=True):
    import torch

    lib, n = env["lib"], len(rows)
    t = np.ascontiguousarray(rows, dtype=np.uint32).reshape(n, 8)
    cp, ckeep = place(t, device)
    fp, fkeep = place(np.frombuffer(fallback, dtype=np.uint8), device) if fallback is not None else (None, None)
    out = ah.Out(n, np.uint8, device)
    rc = lib.zsw_consensus_from_counts(h, cp, n, 1 if device else 0, flags, fp, out.ptr, None)
    assert rc == 0, lib.zsw_last_error_string(h).decode()
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.data().tobytes()


def test_consensus_known_answers_ties_and_uncovered_sites(env):
    from test_pileup_model import tie_table

    _lib, lib = env["_lib"], env["lib"]
    assert (_lib.MEM_HOST, _lib.MEM_DEVICE) == (0, 1)
    known = json.load(open(os.path.join(ROOT, "tests", "golden", "plurality_known_answers.json")))["cases"]
    h = C.c_void_p()
    assert lib.zsw_create(0, C.byref(h)) == 0  # neither scoring nor a sequence is needed
    try:
        rows = [pr.composition(c["input"].encode()) for c in known]
        for device in (True, False):
            assert consensus(env, h, rows, device=device) == "".join(c["expected"] for c in known).encode()
        rows = tie_table() + [[0] * 8, [3, 0, 0, 0, 0, 0, 0, 0], [0] * 8, [0, 0, 0, 0, 0, 9, 9, 9], [0, 0, 0, 0, 1, 0, 0, 0], [0] * 8]  # covered and uncovered sites adjacent
        rows = rows * 5  # more than one block of sites
        fb = bytes((b"acgtn-RY#" * len(rows))[:len(rows)])
        for device in (True, False):
            assert consensus(env, h, rows, device=device) == pr.consensus(rows)
            got = consensus(env, h, rows, pr.KEEP_UNCOVERED, fb, device=device)
            assert got == pr.consensus(rows, pr.KEEP_UNCOVERED, fb)
            assert sum(1 for g, f, r in zip(got, fb, rows) if not any(r[:5]) and g == f) == sum(1 for r in rows if not any(r[:5])) > 10
        assert lib.zsw_consensus_from_counts(h, None, 0, 1, 0, None, None, None) == 0
        cp, keep = place(np.zeros((4, 8), dtype=np.uint32), True)
        out = ah.Out(4, np.uint8, True)
        assert lib.zsw_consensus_from_counts(h, cp, 4, 1, 2, None, out.ptr, None) == -1        # an unknown flag
        assert lib.zsw_consensus_from_counts(h, cp, 4, 1, 1, None, out.ptr, None) == -1        # KEEP_UNCOVERED without a fallback
        assert lib.zsw_consensus_from_counts(h, cp, 4, 1, 0, None, None, None) == -1
        assert lib.zsw_consensus_from_counts(h, cp, 4, 7, 0, None, out.ptr, None) == -1
        assert lib.zsw_consensus_from_counts(h, cp, 4, 1, 0, None, cp + 8, None) == -1         # out_seq over counts
        assert out.untouched()
    finally:
        lib.zsw_destroy(h)


def test_a_refinement_round_stays_on_the_card(env, mixed):
    """pile up, vote with KEEP_UNCOVERED, hand out_seq to zsw_set_reference(ZSW_MEM_DEVICE) and score the same reads again: the
    scores equal those against the host copy of that sequence"""
    import torch

    _lib, lib = env["_lib"], env["lib"]
    ref = bytearray(mixed.ref)
    for k in range(50, 1950, 97):  # the reads come from mixed.ref: the consensus has to repair these
        ref[k] = ord("ACGT"["ACGT".index(chr(ref[k])) ^ 1])
    ref = bytes(ref)
    rs = read_set("refine", ref, mixed.reads[:1500])
    h = ah.new_context(_lib, lib, env["m"], GO, GE, ref)
    try:
        p = ah.Presented(_lib, rs, "device-ragged")
        r, _ = align(env, h, "zsw_align_3pass_batch_from", p, 0)
        pu = Pileup(env, h, p, len(ref), r)
        counts, _, bad = pu.run(pr.CLEAR, base=0)
        assert bad == 0
        fb_ptr, fb_keep = place(np.frombuffer(ref, dtype=np.uint8), True)
        out = ah.Out(len(ref), np.uint8, True)
        assert lib.zsw_consensus_from_counts(h, pu.counts.ptr, len(ref), 1, pr.KEEP_UNCOVERED, fb_ptr, out.ptr, None) == 0
        torch.cuda.synchronize()
        new = out.data().tobytes()
        assert new == pr.consensus(counts, pr.KEEP_UNCOVERED, ref) and out.guards_intact()
        fixed = sum(1 for k in range(50, 1950, 97) if new[k] == mixed.ref[k])
        assert fixed >= 15 and new != ref

        def scores():
            sc, st, tier = ah.Out(rs.n, np.uint32, True), ah.Out(rs.n, np.uint8, True), ah.Out(rs.n, np.uint8, True)
            assert lib.zsw_score_batch_from(h, p.ref(), 8, 256, sc.ptr, st.ptr, tier.ptr, None) == 0
            torch.cuda.synchronize()
            return sc.data(), st.data()

        assert lib.zsw_set_reference(h, out.ptr, len(ref), _lib.MEM_DEVICE) == 0
        on_card = scores()
        buf = np.frombuffer(new, dtype=np.uint8)
        assert lib.zsw_set_reference(h, buf.ctypes.data, len(new), _lib.MEM_HOST) == 0
        from_host = scores()
        assert np.array_equal(on_card[0], from_host[0]) and np.array_equal(on_card[1], from_host[1]) and (on_card[1] == ah.S_).sum() > 1000
    finally:
        lib.zsw_destroy(h)


# ---- errors ----------------------------------------------------------------------------------------------------------------------

def test_argument_errors_write_nothing(env):
    _lib, lib = env["_lib"], env["lib"]
    seq = make_seq(420, 9)
    items = built_items(seq, 150)
    rs = read_set("errors", seq, [it[0] for it in items], 150)
    r = records_of([it[1:] for it in items])
    h = ah.new_context(_lib, lib, env["m"], GO, GE, seq)
    try:
        def refused(p, flags, code, **kw):
            a = Pileup(env, h, p, len(seq), r)
            for k, v in kw.items():
                setattr(a, k, v)
            assert a.call(flags) == code, (code, a.msg())
            import torch

            torch.cuda.synchronize()
            assert a.counts.untouched() and (a.ins is None or a.ins.untouched())
            return a

        packed = ah.Presented(_lib, rs, "host-packed4", lib, h, env["im"])
        refused(packed, 0, -4)                                               # ZSW_ERR_UNSUPPORTED
        p = ah.Presented(_lib, rs, "device-fixed")
        refused(p, 4, -1)                                                    # ZSW_ANNOTATE_MATCH_RESIDUES is not accepted here
        refused(p, 16, -1)                                                   # an unknown flag
        refused(p, pr.SHARED, -5)                                            # no profile sequence
        a = Pileup(env, h, p, len(seq), r)
        a.counts.ptr = a.arrays[0][0]                                        # counts over aln
        assert a.call(0) == -1 and "overlap" in a.msg()
        a = Pileup(env, h, p, len(seq), r)
        a.ins.ptr = a.counts.ptr + 32                                        # ins over counts
        assert a.call(0) == -1 and "overlap" in a.msg() and a.counts.untouched()
        a = Pileup(env, h, p, len(seq), r)
        assert lib.zsw_pileup_batch(h, p.ref(), 0, a.arrays[0][0], a.arrays[1][0], a.arrays[2][0], a.arrays[3][0], len(r.inc), None, None, C.byref(a.n_bad), None) == -1
        assert lib.zsw_pileup_batch(h, p.ref(), 0, a.arrays[0][0], a.arrays[1][0], a.arrays[2][0], a.arrays[3][0], len(r.inc), a.counts.ptr, None, None, None) == -1
        assert lib.zsw_pileup_batch(h, p.ref(), 0, None, a.arrays[1][0], a.arrays[2][0], a.arrays[3][0], len(r.inc), a.counts.ptr, None, C.byref(a.n_bad), None) == -1
        assert a.counts.untouched()
        h2 = C.c_void_p()
        assert lib.zsw_create(0, C.byref(h2)) == 0
        try:
            b = Pileup(env, h2, p, len(seq), r)
            assert b.call(0) == -5 and b.counts.untouched()                  # no reference
        finally:
            lib.zsw_destroy(h2)
    finally:
        lib.zsw_destroy(h)


# ---- the layer above the C ABI ------------------------------------------------------------------------------------------------------

def test_python_pileup_both_roles_strands_and_consensus(env, mixed):
    """zoe_amd: pileup() of the profile classes of both roles (and of a strand-aware call) and plurality_acgtn against pileup_ref"""
    import torch

    za = env["za"]
    reads = [r for r in mixed.reads if r][-400:]
    rc = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    reads = [r.translate(rc)[::-1] if k % 3 == 0 else r for k, r in enumerate(reads)]  # a third from the other strand
    ref = mixed.ref

    def check(aln, got, used_reads, flags, times=1):
        want = pr.pileup(aln.records, aln.status, aln.inc, aln.op, used_reads, ref, flags)
        counts, ins = got
        assert counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (len(ref), 8) and tuple(ins.shape) == (len(ref) + 1, 2)
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), want[0] * np.uint32(times)) and np.array_equal(ins.cpu().numpy().view(np.uint32), want[1])
        return want

    prof = za.into_local_profile(reads, env["m"], GO, GE)
    for src, flags in ((za.SeqSrc.Reference(ref), 0), (za.SeqSrc.Query(ref), ar.READ_IS_REF)):
        aln = prof.sw_align_from_i8_3pass(src)
        counts, ins = prof.pileup(aln, src, insertions=True)
        check(aln, (counts, ins), reads, flags)
        again = prof.pileup(aln, src, counts=counts)                       # accumulates into the table it is given
        assert again is counts
        check(aln, (counts, ins), reads, flags, times=2)
    src = za.SeqSrc.Reference(ref)
    aln = prof.sw_align_strands_from_i8_3pass(src)
    assert aln.strand.any() and not aln.strand.all()
    iupac = bytes.maketrans(b"ACGTURYKMBVDHacgturykmbvdh", b"TGCAAYRMKVBHDtgcaayrmkvbhd")  # the default complement table (include/zoe_sw.h)
    oriented = [r.translate(iupac)[::-1] if s else r for r, s in zip(reads, aln.strand)]
    counts, ins = prof.pileup(aln, src, insertions=True)
    want = check(aln, (counts, ins), oriented, 0)
    cons = za.plurality_acgtn(counts)
    assert cons.is_cuda and cons.dtype == torch.uint8 and cons.cpu().numpy().tobytes() == pr.consensus(want[0])
    assert za.plurality_acgtn(counts, fallback=ref).cpu().numpy().tobytes() == pr.consensus(want[0], pr.KEEP_UNCOVERED, ref)
    assert za.plurality_acgtn(want[0], fallback=ref) == pr.consensus(want[0], pr.KEEP_UNCOVERED, ref)  # a numpy table -> bytes
    shared = za.into_shared_profile(ref, env["m"], GO, GE)
    for src, flags in ((za.SeqBatchSrc.Query(reads), ar.SHARED), (za.SeqBatchSrc.Reference(reads), ar.SHARED | ar.READ_IS_REF)):
        aln = shared.sw_align_from_i8(src)
        check(aln, shared.pileup(aln, src, insertions=True), reads, flags)
