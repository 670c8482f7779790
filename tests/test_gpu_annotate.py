"""GPU tests of zsw_annotate_batch through the C ABI: the device against tests/annotate_ref.py on every record and ciglet.

Shapes are the smallest at which the kernel can go wrong (G = 64 lanes per alignment, 8 alignments per block): read lengths and M
runs around G, reads on both sides of the length that goes through LDS, records of 0 / 1 / G / G + 1 / 70 ciglets, batches of one block +- 1 read and of a few thousand, fixed / ragged / host
presentations, a context sequence on each side of the LDS threshold; then the records of the alignment entry points of both roles
and both `invert` values end to end, the capacity protocol with guard entries, the hand-built malformed records of
tests/test_annotate_model.py (clean there under the sanitizers first), the argument errors and the asynchronous form."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah
import annotate_ref as ar

pytestmark = pytest.mark.gpu

G, BLOCK_READS, LDS_MAX, READ_LDS = 64, 8, 32768, 512  # zsw_annotate.hpp: ANN_G, ANN_LDS_SEQ_MAX; zsw_annotate.hip: ANN_WAVES, ANN_READ_LDS
GO, GE = -10, -1


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
    import os
    import re

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zoe_amd", "csrc")
    hpp, hip = open(os.path.join(csrc, "zsw_annotate.hpp")).read(), open(os.path.join(csrc, "zsw_annotate.hip")).read()
    assert int(re.search(r"ANN_G = (\d+);", hpp).group(1)) == G and int(re.search(r"ANN_LDS_SEQ_MAX = (\d+);", hpp).group(1)) == LDS_MAX
    assert int(re.search(r"ANN_WAVES = (\d+);", hip).group(1)) == BLOCK_READS and int(re.search(r"ANN_READ_LDS = (\d+);", hip).group(1)) == READ_LDS


# ---- one call ------------------------------------------------------------------------------------------------------------------

class Records:
    """caller-side records of a batch: aln (ALN_DTYPE), status, inc, op"""

    def __init__(self, aln, status, inc, op):
        self.aln = np.ascontiguousarray(aln, dtype=ah.ALN_DTYPE)
        self.status = np.ascontiguousarray(status, dtype=np.uint8)
        self.inc = np.ascontiguousarray(inc, dtype=np.uint32)
        self.op = np.ascontiguousarray(op, dtype=np.uint8)


def place(arr: np.ndarray, device: bool):
    """-> (pointer, keep-alive) of a copy of arr where the batch lives"""
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if a.size == 0:
        a = np.zeros(8, dtype=np.uint8)
    if device:
        import torch

        t = torch.from_numpy(a.copy()).cuda()
        return t.data_ptr(), t
    a = a.copy()
    return a.ctypes.data, a


class Annotate:
    """one zsw_annotate_batch call on a presented batch, outputs in guarded arrays"""

    def __init__(self, env, h, p: ah.Presented, flags: int, rec: Records, verbose: bool = True, stream=None):
        self.env, self.h, self.p, self.flags, self.rec, self.verbose, self.stream = env, h, p, flags, rec, verbose, stream
        dev = p.device
        self.n = p.rs.n
        self.ins = [place(a, dev) for a in (rec.aln, rec.status, rec.inc, rec.op)]
        self.stats = ah.Out(self.n, ar.STATS_DTYPE, dev)
        self.aln = ah.Out(self.n, ah.ALN_DTYPE, dev)
        self.total = C.c_uint64(0)
        self.inc = self.op = None

    def call(self, cap, with_arrays=True):
        lib, o = self.env["lib"], self
        if with_arrays and (o.inc is None or o.inc.n != cap):
            o.inc, o.op = ah.Out(cap, np.uint32, o.p.device), ah.Out(cap, np.uint8, o.p.device)
        v = o.verbose
        return lib.zsw_annotate_batch(o.h, o.p.ref(), o.flags, o.ins[0][0], o.ins[1][0], o.ins[2][0], o.ins[3][0], len(o.rec.inc), o.stats.ptr,
                                      o.aln.ptr if v else None, o.inc.ptr if v and with_arrays else None, o.op.ptr if v and with_arrays else None,
                                      cap if v else 0, C.byref(o.total) if v else None, ah.stream_ptr(o.stream))

    def msg(self):
        return self.env["lib"].zsw_last_error_string(self.h).decode()

    def sync(self):
        import torch

        (self.stream.synchronize() if self.stream is not None else torch.cuda.synchronize())

    def outs(self):
        return [a for a in (self.stats, self.aln, self.inc, self.op) if a is not None]

    def run(self):
        """stats only: the one call. Verbose: capacity 0 without arrays -> -1 and the total; total - 1 the same; total succeeds."""
        if not self.verbose:
            assert self.call(0) == 0, self.msg()
            self.sync()
            assert self.stats.guards_intact() and self.aln.untouched()
            return {"stats": self.stats.data()}
        rc0 = self.call(0, with_arrays=False)
        t = int(self.total.value)
        if t == 0:
            assert rc0 == 0, (rc0, self.msg())
        else:
            assert rc0 == -1 and "capacity" in self.msg(), (rc0, self.msg())
            self.total.value = 0
            assert self.call(t - 1) == -1 and int(self.total.value) == t and "capacity" in self.msg()
            self.sync()
            assert self.aln.untouched() and self.inc.untouched() and self.op.untouched(), "a call that failed for capacity wrote records or ciglets"
        self.total.value = 0
        assert self.call(t) == 0, self.msg()
        assert int(self.total.value) == t
        self.sync()
        assert all(a.guards_intact() for a in self.outs()), "guard entries were written"
        return {"stats": self.stats.data(), "aln": self.aln.data(), "inc": self.inc.data(), "op": self.op.data()}


def expect(env, rs: ah.ReadSet, seq: bytes, flags: int, rec: Records):
    stats, out, inc, op = ar.annotate_batch(rec.aln, rec.status, rec.inc, rec.op, rs.reads, seq, flags, env["w"], env["im"], GO, GE)
    return {"stats": stats, "aln": out, "inc": inc, "op": op}


def same(got, want, what):
    for k in got:
        if not np.array_equal(got[k], want[k]):
            bad = np.nonzero(got[k] != want[k])[0] if got[k].shape == want[k].shape else []
            raise AssertionError(f"{what}: `{k}` differs at {len(bad)} entries, first {list(bad[:4])}: got {got[k][bad[:4]]}, want {want[k][bad[:4]]}")


def read_set(name, seq, reads, fixed_len=0):
    n = len(reads)
    return ah.ReadSet(name, seq, [bytes(r) for r in reads], fixed_len, np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64))


def records_of(items):
    """items: per read (status, record dict without ciglet fields or None, [(inc, op)]) -> Records with the ciglets laid out in order"""
    aln = np.zeros(len(items), dtype=ah.ALN_DTYPE)
    status, inc, op = [], [], []
    for i, (st, r, cig) in enumerate(items):
        status.append(st)
        if r is not None:
            for k, v in r.items():
                aln[i][k] = v
        aln[i]["n_ciglets"], aln[i]["ciglet_offset"] = len(cig), len(inc)
        inc += [c[0] for c in cig]
        op += [c[1] for c in cig]
    return Records(aln, status, inc, op)


def rec(rr, qr, ref_len, query_len, score=0):
    return {"score": score, "ref_start": rr[0], "ref_end": rr[1], "query_start": qr[0], "query_end": qr[1], "ref_len": ref_len, "query_len": query_len}


# ---- built shapes ----------------------------------------------------------------------------------------------------------------

def make_seq(n, seed):
    return bytes(ah.ACGT[np.random.default_rng(seed).integers(0, 4, n)])


def built_items(seq: bytes, fixed_len: int = 0):
    """(read, status, record, ciglets) per read, flags 0 (ref = seq, query = read). fixed_len > 0: only reads of that length."""
    R = len(seq)
    out = []

    def add(read, st, r, cigar):
        out.append((bytes(read), st, r, ar.parse_cigar(cigar) if isinstance(cigar, str) else cigar))

    if not fixed_len:
        for L in (1, G - 1, G, G + 1, 150, 401, READ_LDS, READ_LDS + 1):  # one M run over the whole read, a mismatch at its first and last column
            # (reads of up to READ_LDS bases go through LDS, longer ones are read where they are)
            for s in (3, R - L):
                read = bytearray(seq[s:s + L])
                read[0] = read[-1] = ord("n")
                add(read, 0, rec((s, s + L), (0, L), R, L), f"{L}M")
        for run in (1, G, G + 1, 2 * G + 3):  # a mismatch on each side of every sweep boundary, at the first and last column of a run
            for bad in ([], [0], [run - 1], sorted({k for b in range(G, run, G) for k in (b - 1, b)}), [b - 1 for b in range(G, run + 1, G)], list(range(G, run, G))):
                read = bytearray(seq[7:7 + 5 + run + 4])
                for k in bad:
                    read[5 + k] = ord("a")
                read[4] = ord("c")
                add(read, 0, rec((12, 12 + run), (5, 5 + run), R, len(read)), f"5S{run}M4S")
                add(read, 0, rec((10, 14 + run), (3, 7 + run), R, len(read)), f"3S2X{run}M2=2S")
        add(b"", 3, None, [])                                    # an empty read
        add(seq[40:190], 2, None, [])                            # a read without an alignment
        add(seq[40:190], 0, rec((40, 40), (0, 0), R, 150), [])   # SOME with no ciglets: the query is not used
    L = fixed_len or 150
    base = seq[50:50 + L]
    for pairs in (1, (G - 1) // 2, G // 2, 35):                  # 1 + 2 * pairs ciglets: 3, G - 1, G + 1, 71; G and 70 below
        read = bytearray()
        for k in range(pairs):
            read += bytes([base[k], ord("T")])
        read += base[pairs:]
        read = bytes(read[:L])  # the tail of the reference piece falls off: the record ends earlier
        used = L - 2 * pairs + pairs
        add(read, 0, rec((50, 50 + used), (0, L), R, L), "1M1I" * pairs + f"{L - 2 * pairs}M")
    add(base, 0, rec((50, 50 + L), (0, L), R, L), "1=1X" * (G // 2) + f"{L - G}M")  # G + 1 ciglets, caller-built = / X
    add(base, 0, rec((50, 50 + L), (0, L), R, L), "1=1X" * 34 + f"1={L - 69}M")   # 70 ciglets
    add(base, 0, rec((50, 50 + L), (0, L), R, L), "1M" * G)                        # G ciglets of one column, too short for the read
    add(base, 0, rec((50, 50 + L), (0, L), R, L), f"3=2M{L - 5}=")                 # the merge across ciglets
    add(base, 0, rec((50, 50 + L), (0, L), R, L), f"{L}M")
    return out


def run_built(env, seq, items, pres, fixed_len=0, verbose=True, flags=0):
    _lib, lib = env["_lib"], env["lib"]
    h = ah.new_context(_lib, lib, env["m"], GO, GE, seq)
    try:
        rs = read_set("built", seq, [it[0] for it in items], fixed_len)
        r = records_of([it[1:] for it in items])
        want = expect(env, rs, seq, flags, r)
        for pr in pres:
            got = Annotate(env, h, ah.Presented(_lib, rs, pr), flags, r, verbose).run()
            same(got, {k: want[k] for k in got}, f"{pr} n={rs.n}")
        return want
    finally:
        lib.zsw_destroy(h)


def test_built_shapes_ragged_and_host(env):
    seq = make_seq(700, 5)
    items = built_items(seq)
    want = run_built(env, seq, items, ("device-ragged", "host-ragged"))
    st = want["stats"]["path_status"]
    assert {ar.OK, ar.NEGATIVE_SCORE, ar.NO_ALIGNMENT, ar.FULL_QUERY_NOT_USED} <= set(int(x) for x in st)
    assert int(want["aln"]["n_ciglets"].max()) >= 70
    run_built(env, seq, items, ("device-ragged",), verbose=False)


def test_built_shapes_fixed_and_both_equalities(env):
    seq = make_seq(420, 6)
    items = built_items(seq, 150)
    for flags in (0, ar.MATCH_RESIDUES):
        run_built(env, seq, items, ("device-fixed", "host-fixed", "device-ragged"), fixed_len=150, flags=flags)


@pytest.mark.parametrize("n", [1, BLOCK_READS - 1, BLOCK_READS, BLOCK_READS + 1, 3000])
def test_batch_sizes(env, n):
    seq = make_seq(700, 7)
    items = built_items(seq)
    items = [items[(k * 7) % len(items)] for k in range(n)]
    run_built(env, seq, items, ("device-ragged",))


@pytest.mark.parametrize("R", [LDS_MAX, LDS_MAX + 1])
def test_both_sides_of_the_lds_threshold(env, R):
    """a context sequence that is staged in LDS whole, and one that is one byte too long and read through L2: reads cut from its
    first and its last bases"""
    seq = make_seq(R, 8)
    items = []
    for s, L in ((0, 150), (R - 150, 150), (R - 65, 65), (R - 1, 1), (LDS_MAX - 100, 100), (R // 2, 401)):
        read = bytearray(seq[s:s + L])
        read[L // 2] = ord("n")
        items.append((bytes(read), 0, rec((s, s + L), (0, L), R, L), ar.parse_cigar(f"{L}M")))
        clips = (f"{s}S" if s else "", f"{R - s - L}S" if R - s - L else "")
        items.append((bytes(read), 0, rec((0, L), (s, s + L), L, R), ar.parse_cigar(f"{clips[0]}{L}M{clips[1]}")))  # the inverted record
    fwd, inv = items[0::2], items[1::2]
    w = run_built(env, seq, fwd, ("device-ragged", "host-ragged"))
    assert (w["stats"]["path_status"] == ar.OK).all() and (w["stats"]["mismatches"] == 1).all()
    w = run_built(env, seq, inv, ("device-ragged",), flags=ar.READ_IS_REF)
    assert (w["stats"]["path_status"] == ar.OK).all() and (w["stats"]["mismatches"] == 1).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------

ENTRY_POINTS = ("zsw_align_batch_from", "zsw_align_3pass_batch_from", "zsw_align_3pass_strands_batch_from", "zsw_align_shared_batch_from",
                "zsw_align_3pass_shared_batch_from")


@pytest.fixture(scope="module")
def mixed(env):
    from zoe_amd import synth

    ref = bytes(synth.reference_host(2000))
    rs = ah.mixed_set("annotate-mixed", ref, 220, 0, 20261020)
    want = {"near", "one_indel", "indels", "ties", "bytes", "all_n", "empty"}
    assert want <= {ah.CLASSES[c] for c in rs.cls}
    return rs


def align(env, h, name, p, invert):
    """the records of an alignment entry point on a device batch -> (Records, strand or None)"""
    import torch

    lib, n = env["lib"], p.rs.n
    aln, status, tier, strand = (ah.Out(n, dt, True) for dt in (ah.ALN_DTYPE, np.uint8, np.uint8, np.uint8))
    total = C.c_uint64(0)
    cap = 64 * n
    inc, op = ah.Out(cap, np.uint32, True), ah.Out(cap, np.uint8, True)
    args = [h, p.ref(), 8, 256, invert, aln.ptr, status.ptr, tier.ptr]
    if "strands" in name:
        args.append(strand.ptr)
    rc = getattr(lib, name)(*args, inc.ptr, op.ptr, cap, C.byref(total), None)
    assert rc == 0, (name, rc, lib.zsw_last_error_string(h).decode())
    torch.cuda.synchronize()
    t = int(total.value)
    return Records(aln.data(), status.data(), inc.data()[:t], op.data()[:t]), (strand.data() if "strands" in name else None)


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_end_to_end(env, mixed, name, invert):
    """the records of every alignment entry point: device annotate == annotate_ref on every record and ciglet under both equalities;
    every SOME record walks to ZSW_PATH_OK with path_score == score (SURVEY 8c on every CIGAR); the counts add up to the ranges; the
    verbose CIGAR folds back to the input"""
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
        if strand is not None:  # annotate the batch as aligned: zsw_orient_batch
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
        assert some.sum() > 150
        for eq in (0, ar.MATCH_RESIDUES):
            got = Annotate(env, h, p, flags | eq, r).run()
            same(got, expect(env, rs, mixed.ref, flags | eq, r), f"{name} invert={invert} eq={eq}")
            s, a = got["stats"], r.aln
            assert (s["path_status"][some] == ar.OK).all() and (s["path_status"][~some] == ar.NO_ALIGNMENT).all()
            assert np.array_equal(s["path_score"][some].astype(np.int64), a["score"][some].astype(np.int64))
            cols = s["matches"].astype(np.int64) + s["mismatches"]
            assert np.array_equal((cols + s["ins_bases"])[some], (a["query_end"].astype(np.int64) - a["query_start"])[some])
            assert np.array_equal((cols + s["del_bases"])[some], (a["ref_end"].astype(np.int64) - a["ref_start"])[some])
            for i in np.nonzero(some)[0]:
                v = got["aln"][i]
                folded = []
                for k in range(int(v["ciglet_offset"]), int(v["ciglet_offset"]) + int(v["n_ciglets"])):
                    ar.add_ciglet(folded, int(got["inc"][k]), ord("M") if got["op"][k] in b"=X" else int(got["op"][k]))
                o, m = int(a[i]["ciglet_offset"]), int(a[i]["n_ciglets"])
                assert folded == [(int(r.inc[o + k]), int(r.op[o + k])) for k in range(m)], i
            for f in ("score", "ref_start", "ref_end", "query_start", "query_end", "ref_len", "query_len"):
                assert np.array_equal(got["aln"][f], a[f])
        gaps = (got["stats"]["ins_runs"] + got["stats"]["del_runs"])[some]
        assert gaps.max() >= 1
    finally:
        lib.zsw_destroy(h)


# ---- malformed records -----------------------------------------------------------------------------------------------------------

def test_malformed_records_are_statuses(env):
    """the hand-built records of tests/test_annotate_model.py (every ZSW_PATH_* status; clean there under address and undefined-behaviour
    sanitizers through the same header) in one batch, good reads between them: every status as on the CPU, every other read as alone"""
    from test_annotate_model import READ, SEQ, status_cases

    _lib, lib = env["_lib"], env["lib"]
    cases = [(w, c) for w, c in status_cases() if c["flags"] == 0]
    # every case brings the whole ciglet arrays of its own call; in one call they follow each other, and the record whose ciglets
    # pass the end of its arrays goes last, so that they pass the end of these
    past = [k for k, (_, c) in enumerate(cases) if c["rec"]["ciglet_offset"] + c["rec"]["n_ciglets"] > len(c["inc"]) and c["rec"]["ciglet_offset"] < 2 ** 32]
    assert len(past) == 1
    cases.append(cases.pop(past[0]))
    good = (0, {**rec((20, 120), (0, 100), len(SEQ), len(READ), 200)}, [(100, ord("M"))])
    reads, labels = [], []
    aln = np.zeros(2 * len(cases), dtype=ah.ALN_DTYPE)
    status, inc, op = [], [], []
    for k, (w, c) in enumerate(cases):
        for which in ("case", "good"):
            i = len(reads)
            if which == "case":
                reads.append(c["read"])
                for f, v in c["rec"].items():
                    aln[i][f] = v % 2 ** 64 if f == "ciglet_offset" else v
                if c["rec"]["ciglet_offset"] < 2 ** 32:
                    aln[i]["ciglet_offset"] = c["rec"]["ciglet_offset"] + len(inc)
                status.append(c["status"])
                inc += c["inc"]
                op += c["op"]
                labels.append(w)
            elif k + 1 < len(cases):  # (nothing behind the last case: its ciglets must pass the end)
                reads.append(READ)
                for f, v in good[1].items():
                    aln[i][f] = v
                aln[i]["n_ciglets"], aln[i]["ciglet_offset"] = 1, len(inc)
                status.append(0)
                inc.append(100)
                op.append(ord("M"))
                labels.append(ar.OK)
    n = len(reads)
    r = Records(aln[:n], status, inc, op)
    rs = read_set("malformed", SEQ, reads)
    h = ah.new_context(_lib, lib, env["m"], GO, GE, SEQ)
    try:
        got = Annotate(env, h, ah.Presented(_lib, rs, "device-ragged"), 0, r).run()
        same(got, expect(env, rs, SEQ, 0, r), "malformed")
        assert [int(x) for x in got["stats"]["path_status"]] == labels
        assert set(labels) == set(range(9))
        goods = np.array([k % 2 == 1 for k in range(n)])
        assert (got["stats"]["matches"][goods] == 100).all() and (got["stats"]["path_score"][goods] == 200).all() and (got["aln"]["n_ciglets"][goods] == 1).all()
    finally:
        lib.zsw_destroy(h)


# ---- errors and asynchrony -------------------------------------------------------------------------------------------------------

def test_argument_errors_write_nothing(env):
    _lib, lib = env["_lib"], env["lib"]
    seq = make_seq(420, 9)
    items = built_items(seq, 150)
    rs = read_set("errors", seq, [it[0] for it in items], 150)
    r = records_of([it[1:] for it in items])
    h = ah.new_context(_lib, lib, env["m"], GO, GE, seq)
    try:
        def refused(p, flags, code):
            a = Annotate(env, h, p, flags, r)
            a.inc, a.op = ah.Out(4096, np.uint32, p.device), ah.Out(4096, np.uint8, p.device)
            assert a.call(4096) == code, (code, a.msg())
            a.sync()
            assert all(o.untouched() for o in a.outs()) and a.total.value == 0

        packed = ah.Presented(_lib, rs, "host-packed4", lib, h, env["im"])
        refused(packed, 0, -4)                                               # ZSW_ERR_UNSUPPORTED
        p = ah.Presented(_lib, rs, "device-fixed")
        refused(p, 8, -1)                                                    # an unknown flag
        refused(p, ar.SHARED, -5)                                            # no profile sequence
        a = Annotate(env, h, p, 0, r)
        a.inc, a.op = ah.Out(4096, np.uint32, True), ah.Out(4096, np.uint8, True)
        a.aln.ptr = a.ins[0][0]                                              # out_aln over aln
        assert a.call(4096) == -1 and "overlap" in a.msg()
        h2 = C.c_void_p()
        assert lib.zsw_create(0, C.byref(h2)) == 0
        try:
            b = Annotate(env, h2, p, 0, r)
            b.inc, b.op = ah.Out(16, np.uint32, True), ah.Out(16, np.uint8, True)
            assert b.call(16) == -5                                          # no scoring
            assert all(o.untouched() for o in b.outs())
        finally:
            lib.zsw_destroy(h2)
    finally:
        lib.zsw_destroy(h)


def test_asynchronous_stats_then_an_alignment_on_the_same_stream(env, mixed):
    import torch

    _lib, lib = env["_lib"], env["lib"]
    h = ah.new_context(_lib, lib, env["m"], GO, GE, mixed.ref)
    try:
        p = ah.Presented(_lib, mixed, "device-ragged")
        r, _ = align(env, h, "zsw_align_3pass_batch_from", p, 0)
        sync_stats = Annotate(env, h, p, 0, r, verbose=False).run()["stats"]
        stream = torch.cuda.Stream()
        a = Annotate(env, h, p, 0, r, verbose=False, stream=stream)
        e = ah.ENTRY["zsw_align_3pass_batch_from"]
        assert a.call(0) == 0, a.msg()                                       # queued, not waited for
        c = ah.Call(_lib, lib, h, e, p, stream=stream).run()
        res = c.collect()
        a.sync()
        assert np.array_equal(a.stats.data(), sync_stats) and a.stats.guards_intact() and a.aln.untouched()
        assert np.array_equal(res["aln"], r.aln) and np.array_equal(res["status"], r.status) and np.array_equal(res["inc"], r.inc)
    finally:
        lib.zsw_destroy(h)


# ---- the layers above the C ABI ----------------------------------------------------------------------------------------------------

def test_python_annotate_both_roles_and_strands(env, mixed):
    """zoe_amd: annotate() of the profile classes of both roles (and of a strand-aware call) against annotate_ref, AlignmentBatch.nm"""
    za = env["za"]
    reads = [r for r in mixed.reads if r][:120]
    rc = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    reads = [r.translate(rc)[::-1] if k % 3 == 0 else r for k, r in enumerate(reads)]  # a third from the other strand
    ref = mixed.ref

    def check(aln, stats, verbose, used_reads, flags):
        want_s, want_a, want_i, want_o = ar.annotate_batch(aln.records, aln.status, aln.inc, aln.op, used_reads, ref, flags, env["w"], env["im"], GO, GE)
        assert stats.dtype == za.STATS_DTYPE and np.array_equal(stats, want_s.astype(za.STATS_DTYPE))
        assert np.array_equal(za.AlignmentBatch.nm(stats), want_s["mismatches"] + want_s["ins_bases"] + want_s["del_bases"])
        if verbose is not None:
            assert np.array_equal(verbose.records, want_a) and np.array_equal(verbose.inc, want_i) and np.array_equal(verbose.op, want_o)
            assert np.array_equal(verbose.status, aln.status)

    prof = za.into_local_profile(reads, env["m"], GO, GE)
    for src, flags in ((za.SeqSrc.Reference(ref), 0), (za.SeqSrc.Query(ref), ar.READ_IS_REF)):
        aln = prof.sw_align_from_i8_3pass(src)
        verbose, stats = prof.annotate(aln, src)
        check(aln, stats, verbose, reads, flags)
        none, stats2 = prof.annotate(aln, src, residues=True, verbose=False)
        assert none is None
        check(aln, stats2, None, reads, flags | ar.MATCH_RESIDUES)
    src = za.SeqSrc.Reference(ref)
    aln = prof.sw_align_strands_from_i8_3pass(src)
    assert aln.strand.any() and not aln.strand.all()
    verbose, stats = prof.annotate(aln, src)
    iupac = bytes.maketrans(b"ACGTURYKMBVDHacgturykmbvdh", b"TGCAAYRMKVBHDtgcaayrmkvbhd")  # the default complement table (include/zoe_sw.h)
    oriented = [r.translate(iupac)[::-1] if s else r for r, s in zip(reads, aln.strand)]
    check(aln, stats, verbose, oriented, 0)
    some = aln.status == 0
    assert (stats["path_status"][some] == ar.OK).all() and np.array_equal(stats["path_score"][some], aln.records["score"][some].astype(np.int32))
    shared = za.into_shared_profile(ref, env["m"], GO, GE)
    for src, flags in ((za.SeqBatchSrc.Query(reads), ar.SHARED), (za.SeqBatchSrc.Reference(reads), ar.SHARED | ar.READ_IS_REF)):
        aln = shared.sw_align_from_i8(src)
        verbose, stats = shared.annotate(aln, src)
        check(aln, stats, verbose, reads, flags)


def test_driver_nm_and_verbose_cigar(env, tmp_path):
    """examples/zsw_driver --3pass --nm --verbose-cigar: NM:i: and the CIGAR column equal zoe_amd.records with the same switches; without
    the switches every line is what zoe_amd.records writes without them (AS:i: alone, M CIGARs)"""
    import os
    import subprocess

    from zoe_amd import build, records, synth

    exe = build.build_driver()
    ref = synth.reference_host(1200)
    reads = synth.reads_host(ref, 4242, 200, 100)
    reads[3] = ord("N")
    (tmp_path / "ref.fa").write_bytes(b">synthref test\n" + ref + b"\n")
    with open(tmp_path / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d extra\n" % i + r.tobytes() + b"\n+\n" + b"I" * len(r) + b"\n")
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(__import__("torch").__file__), "lib") + ":" + e.get("LD_LIBRARY_PATH", "")
    fq = list(records.FastQReader.from_path(str(tmp_path / "reads.fq")))

    def driver(*switches):
        out = subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), "--3pass", *switches], capture_output=True, text=True, env=e, timeout=300)
        assert out.returncode == 0, out.stderr
        return [line for line in out.stdout.splitlines() if not line.startswith("@")]

    plain = driver()
    assert plain == [str(s) for s in records.align_fastq_to_sam(fq, ref, "synthref", env["m"], GO, GE, three_pass=True)]
    assert all("NM:i:" not in line and "=" not in line.split("\t")[5] for line in plain)
    for switches, kw in ((("--nm", "--verbose-cigar"), {"nm": True, "verbose_cigar": True}), (("--nm",), {"nm": True}), (("--verbose-cigar",), {"verbose_cigar": True})):
        got = driver(*switches)
        want = [str(s) for s in records.align_fastq_to_sam(fq, ref, "synthref", env["m"], GO, GE, three_pass=True, **kw)]
        assert got == want, switches
        mapped = [line.split("\t") for line in got if line.split("\t")[1] == "0"]
        assert len(mapped) > 150
        if "--nm" in switches:
            assert all(f[12].startswith("NM:i:") for f in mapped) and any(f[12] != "NM:i:0" for f in mapped)
        if "--verbose-cigar" in switches:
            assert all("M" not in f[5] for f in mapped) and any("X" in f[5] for f in mapped)
            assert [f[:5] + f[6:12] for f in mapped] == [f[:5] + f[6:12] for f in (line.split("\t") for line in plain) if f[1] == "0"]
