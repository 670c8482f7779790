"""GPU tests of zsw_sam_batch through the C ABI and the layers above it: the device against tests/sam_ref.py, byte for byte, on the
text and on out_line_offsets.

Shapes are the smallest at which the kernel can go wrong (64 lanes per line, SAM_BLOCK_LINES lines per block, lines of up to
SAM_LDS_LINE bytes assembled in LDS and flushed in 16-byte granules): the shape list of tests/sam_cases.py (clean in the host model
first, tests/test_sam_model.py) as device and host batches, fixed and ragged, with names of 0..31 bytes in a row so that line
starts fall on every residue mod 16; batches of one block +- 1 line and of 3,000; the capacity protocol with sentinel bytes behind
the text and an unaligned buffer; two runs; the records of the alignment entry points end to end, with strands and with the
annotation's verbose records and stats; one stream without a host synchronise; the argument errors; the Python and C++ layers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_helpers as ah
import sam_cases as sc
import sam_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_sam.hpp")).read()
BLOCK_LINES = int(re.search(r"SAM_BLOCK_LINES = (\d+);", HPP).group(1))
LDS_LINE = int(re.search(r"SAM_LDS_LINE = (\d+);", HPP).group(1))
STATS_DTYPE = np.dtype([("matches", "<u4"), ("mismatches", "<u4"), ("ins_bases", "<u4"), ("del_bases", "<u4"), ("ins_runs", "<u4"), ("del_runs", "<u4"),
                        ("path_score", "<i4"), ("path_status", "<u4")])
SENTINEL = 0xA5
TAIL = 64
GO, GE = -10, -1


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib, synth

    lib = _lib.load()
    assert hasattr(lib, "zsw_sam_batch")
    m = zoe_amd.WeightMatrix.new(zoe_amd.DNA_PROFILE_MAP, 2, -5, b"N")
    ref = synth.reference_host(2000)
    h = ah.new_context(_lib, lib, m, GO, GE, ref)
    yield {"za": zoe_amd, "_lib": _lib, "lib": lib, "m": m, "ref": ref, "h": h}
    lib.zsw_destroy(h)


def place(arr, device: bool):
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


class Batch:
    """what one zsw_sam_batch call is given, on the host: reads, records, and the optional arrays (None = absent)"""

    def __init__(self, reads, aln, status, inc, op, names=None, quals=None, strand=None, stats=None, rname=sc.RNAME, mapq=255, omit_seq=False, fixed_len=0):
        self.reads = [bytes(r) for r in reads]
        self.aln = np.ascontiguousarray(aln, dtype=ah.ALN_DTYPE)
        self.status = np.ascontiguousarray(status, dtype=np.uint8)
        self.inc = np.ascontiguousarray(inc, dtype=np.uint32)
        self.op = np.ascontiguousarray(op, dtype=np.uint8)
        self.names, self.quals, self.rname, self.mapq, self.omit_seq, self.fixed_len = names, quals, bytes(rname), mapq, omit_seq, fixed_len
        self.strand = None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)
        self.stats = None if stats is None else np.ascontiguousarray(stats, dtype=STATS_DTYPE)
        self.n = len(self.reads)

    def expected(self):
        """-> (text, line offsets, malformed records) by tests/sam_ref.py"""
        lines, n_bad = [], 0
        for i in range(self.n):
            st = None if self.stats is None else (int(self.stats[i]["mismatches"]), int(self.stats[i]["ins_bases"]), int(self.stats[i]["del_bases"]))
            line, bad = sam_ref.sam_line(None if self.names is None else self.names[i], self.reads[i], None if self.quals is None else self.quals[i],
                                         int(self.status[i]), self.aln[i], self.inc, self.op, self.rname, self.mapq,
                                         0 if self.strand is None else int(self.strand[i]), st, self.omit_seq)
            lines.append(line)
            n_bad += bad
        off = np.zeros(self.n + 1, dtype=np.uint64)
        np.cumsum([len(l) for l in lines], out=off[1:])
        return b"".join(lines), off, n_bad


class Sam:
    """one presented batch and its zsw_sam_batch calls"""

    def __init__(self, env, b: Batch, pres: str, stream=None, device_records=None):
        self.env, self.b, self.stream = env, b, stream
        rs = ah.ReadSet("sam", b"", b.reads, b.fixed_len, np.zeros(b.n, dtype=np.int64), np.full(b.n, -1, dtype=np.int64))
        self.p = p = ah.Presented(env["_lib"], rs, pres)
        dev = p.device
        self.keep = []

        def put(a):
            ptr, k = place(a, dev)
            self.keep.append(k)
            return ptr

        if device_records is not None:  # pointers to device arrays an earlier call wrote
            self.rec_ptrs = device_records
        else:
            self.rec_ptrs = [put(b.aln), put(b.status), put(b.inc), put(b.op)]
        f = env["_lib"].ZswSamFields()
        if b.names is not None:
            noff = np.zeros(b.n + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in b.names], out=noff[1:])
            f.qnames, f.qname_offsets = put(np.frombuffer(b"".join(b.names) or b"\0", dtype=np.uint8)), put(noff)
        if b.quals is not None:
            f.quals = put(np.frombuffer(b"".join(b.quals) or b"\0", dtype=np.uint8))
        if b.strand is not None:
            f.strand = put(b.strand)
        if b.stats is not None:
            f.stats = put(b.stats)
        f.rname, f.rname_len, f.mapq = b.rname, len(b.rname), b.mapq
        self.f = f
        self.flags = env["_lib"].SAM_OMIT_SEQ if b.omit_seq else 0
        self.total, self.n_bad = C.c_uint64(0), C.c_uint64(0)

    def call(self, text_ptr, cap, off_ptr=None, flags=None, fields=None, recs=None):
        r = self.rec_ptrs if recs is None else recs
        return self.env["lib"].zsw_sam_batch(self.env["h"], self.p.ref(), C.byref(self.f if fields is None else fields), self.flags if flags is None else flags,
                                             r[0], r[1], r[2], r[3], len(self.b.inc), text_ptr, cap, C.byref(self.total), off_ptr, C.byref(self.n_bad),
                                             ah.stream_ptr(self.stream))

    def msg(self):
        return self.env["lib"].zsw_last_error_string(self.env["h"]).decode()

    def sync(self):
        import torch

        (self.stream.synchronize() if self.stream is not None else torch.cuda.synchronize())

    def buffer(self, nbytes, shift=0):
        """`nbytes` bytes of SENTINEL in the batch's memory, starting `shift` bytes into their allocation -> (pointer, fetch())"""
        raw = np.full(nbytes + shift, SENTINEL, dtype=np.uint8)
        if self.p.device:
            import torch

            t = torch.from_numpy(raw).cuda()
            assert t.data_ptr() % 16 == 0
            return t.data_ptr() + shift, lambda: t.cpu().numpy()[shift:]
        return raw.ctypes.data + shift, lambda: raw[shift:]

    def run(self, shift=0):
        """sizing call, then the call with exactly the capacity it asked for -> (text, line offsets, n_bad); the TAIL bytes behind
        the text and the guards of the offsets must stay as they were"""
        assert self.call(None, 0) == 0, self.msg()
        total = int(self.total.value)
        ptr, fetch = self.buffer(total + TAIL, shift)
        off = ah.Out(self.b.n + 1, np.uint64, self.p.device)
        self.total.value = 0
        assert self.call(ptr, total, off.ptr) == 0, self.msg()
        self.sync()
        got = fetch()
        assert int(self.total.value) == total
        assert (got[total:] == SENTINEL).all(), "bytes behind out_text[total] were written"
        assert off.guards_intact()
        return got[:total].tobytes(), off.data(), int(self.n_bad.value)


def check(env, b: Batch, pres: str, shift=0):
    text, off, n_bad = b.expected()
    got = Sam(env, b, pres).run(shift)
    if got[0] != text:
        gl, wl = got[0].split(b"\n"), text.split(b"\n")
        k = next((i for i, (x, y) in enumerate(zip(gl, wl)) if x != y), min(len(gl), len(wl)))
        raise AssertionError(f"{pres}: line {k} differs:\n got {gl[k:k + 1]}\nwant {wl[k:k + 1]}")
    assert np.array_equal(got[1], off), pres
    assert got[2] == n_bad, (pres, got[2], n_bad)
    return got


def test_the_constants_the_shapes_are_built_from():
    assert BLOCK_LINES >= 2 and LDS_LINE >= 256 and int(re.search(r"SAM_G = (\d+);", HPP).group(1)) == 64


# ---- built records ---------------------------------------------------------------------------------------------------------------

def batch_of(cases, cfg, fixed_len=0, **kw):
    names, quals, strand, stats, omit = cfg
    recs, inc, op = sc.assemble(cases)
    aln = np.zeros(len(cases), dtype=ah.ALN_DTYPE)
    st = np.zeros(len(cases), dtype=STATS_DTYPE)
    for k, (c, r) in enumerate(zip(cases, recs)):
        for key in ("score", "ref_start", "n_ciglets", "ciglet_offset"):
            aln[k][key] = r[key]
        st[k]["mismatches"], st[k]["ins_bases"], st[k]["del_bases"] = c["stats"]
    return Batch([c["read"] for c in cases], aln, [c["status"] for c in cases], inc, op, [c["name"] for c in cases] if names else None,
                 [c["qual"] for c in cases] if quals else None, [c["strand"] for c in cases] if strand else None, st if stats else None, omit_seq=omit,
                 fixed_len=fixed_len, **kw)


CFG_IDS = ["".join("NQSTO"[k] if on else "-" for k, on in enumerate(c)) for c in sc.CONFIGS]


@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("pres", ["device-ragged", "host-ragged"])
def test_the_shape_list_ragged(env, pres, cfg):
    cases = sc.shape_cases(LDS_LINE, cfg)
    got = check(env, batch_of(cases, cfg), pres)
    assert got[2] == 9  # the malformed records built in
    if cfg == sc.CONFIGS[0]:
        assert {int(x) % 16 for x in got[1]} == set(range(16))  # line starts on every residue mod 16
        assert {LDS_LINE - 1, LDS_LINE, LDS_LINE + 1} <= {int(x) for x in np.diff(got[1])}


@pytest.mark.parametrize("cfg", [sc.CONFIGS[0], sc.CONFIGS[-1]], ids=[CFG_IDS[0], CFG_IDS[-1]])
@pytest.mark.parametrize("pres", ["device-fixed", "host-fixed"])
def test_the_shape_list_fixed(env, pres, cfg):
    cases = [c for c in sc.shape_cases(LDS_LINE, cfg) if len(c["read"]) == 37]
    assert len(cases) > 50
    assert check(env, batch_of(cases, cfg, fixed_len=37), pres)[2] == 9


def test_zero_length_reads_have_stars(env):
    """the one intended difference from the driver's host loop: `*` for SEQ and QUAL of a read of length 0"""
    cases = [sc.case(b"a", read=b"", status=0), sc.case(b"b", read=b"", status=2), sc.case(b"c", read=b"AC", status=0)]
    text = check(env, batch_of(cases, sc.CONFIGS[0]), "device-ragged")[0].split(b"\n")
    assert text[0].split(b"\t")[9:11] == [b"*", b"*"] and text[1].split(b"\t")[9:11] == [b"*", b"*"] and text[2].split(b"\t")[9] == b"AC"


# ---- batch sizes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, BLOCK_LINES - 1, BLOCK_LINES, BLOCK_LINES + 1, 3000])
def test_batch_sizes(env, n):
    pool = sc.shape_cases(LDS_LINE)
    cases = [pool[(5 * k) % len(pool)] for k in range(n)]
    check(env, batch_of(cases, sc.CONFIGS[0]), "device-ragged")


# ---- capacity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pres,shift", [("device-ragged", 0), ("device-ragged", 1), ("device-ragged", 2), ("device-ragged", 3), ("host-ragged", 1)])
def test_capacity_protocol(env, pres, shift):
    cases = sc.shape_cases(LDS_LINE)[:60]
    b = batch_of(cases, sc.CONFIGS[0])
    text, off, _ = b.expected()
    total = len(text)
    s = Sam(env, b, pres)
    assert s.call(None, 0) == 0 and int(s.total.value) == total  # the sizing call
    ptr, fetch = s.buffer(total + TAIL, shift)
    offs = ah.Out(b.n + 1, np.uint64, s.p.device)
    s.total.value = 0
    assert s.call(ptr, total - 1, offs.ptr) == -1 and "capacity" in s.msg()
    s.sync()
    assert int(s.total.value) == total
    assert (fetch() == SENTINEL).all(), "a call that failed for capacity wrote text"
    assert np.array_equal(offs.data(), off) and offs.guards_intact()  # the offsets are written all the same
    assert s.call(ptr, total, offs.ptr) == 0, s.msg()
    s.sync()
    got = fetch()
    assert got[:total].tobytes() == text and (got[total:] == SENTINEL).all()
    check(env, b, pres, shift)


def test_two_calls_give_identical_bytes(env):
    b = batch_of([sc.shape_cases(LDS_LINE)[(7 * k) % 70] for k in range(500)], sc.CONFIGS[0])
    s = Sam(env, b, "device-ragged")
    first, second = s.run(), s.run()
    assert first[0] == second[0] == b.expected()[0] and np.array_equal(first[1], second[1]) and first[2] == second[2]


# ---- end to end ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(env):
    rs = ah.mixed_set("sam-mixed", env["ref"], 2000, 0, 20240521)
    assert sum(len(r) == 0 for r in rs.reads) > 10
    names = [b"m%d/%d" % (i, i % 7) for i in range(rs.n)]
    quals = [bytes(33 + (i + 3 * k) % 60 for k in range(len(r))) for i, r in enumerate(rs.reads)]
    return rs, names, quals


def aligned(env, rs, entry):
    p = ah.Presented(env["_lib"], rs, "device-ragged")
    return ah.Call(env["_lib"], env["lib"], env["h"], ah.ENTRY[entry], p).run().collect()


@pytest.mark.parametrize("entry", ["zsw_align_batch_from", "zsw_align_3pass_batch_from"])
@pytest.mark.parametrize("annotate", [False, True], ids=["plain", "verbose+NM"])
def test_end_to_end(env, mixed, entry, annotate):
    rs, names, quals = mixed
    res = aligned(env, rs, entry)
    assert 50 < (res["status"] != 0).sum() < rs.n - 500  # some unmapped, most mapped
    stats = None
    if annotate:
        res, stats = annotated(env, rs.reads, res)
        assert b"=" in res["op"].tobytes() and b"X" in res["op"].tobytes()
    b = Batch(rs.reads, res["aln"], res["status"], res["inc"], res["op"], names, quals, None, stats, rname=b"synthref")
    got = check(env, b, "device-ragged")
    assert got[2] == 0
    line = got[0].split(b"\n")[int(np.nonzero(res["status"] == 0)[0][0])].split(b"\t")
    assert line[1] == b"0" and line[2] == b"synthref" and line[11].startswith(b"AS:i:") and (len(line) == 13 and line[12].startswith(b"NM:i:") if annotate else len(line) == 12)
    check(env, b, "host-ragged")


def annotated(env, reads, res, flags=0):
    """zsw_annotate_batch (verbose) over the records of an alignment call -> (its verbose records, its stats)"""
    import torch

    lib, h = env["lib"], env["h"]
    rs = ah.ReadSet("ann", b"", list(reads), 0, np.zeros(len(reads), dtype=np.int64), np.full(len(reads), -1, dtype=np.int64))
    p = ah.Presented(env["_lib"], rs, "device-ragged")
    ins = [place(res[k], True) for k in ("aln", "status", "inc", "op")]
    n = rs.n
    stats, out = ah.Out(n, STATS_DTYPE, True), ah.Out(n, ah.ALN_DTYPE, True)
    total = C.c_uint64(0)
    call = lambda i, o, cap: lib.zsw_annotate_batch(h, p.ref(), flags, ins[0][0], ins[1][0], ins[2][0], ins[3][0], len(res["inc"]), stats.ptr, out.ptr, i, o, cap,
                                                    C.byref(total), None)
    assert call(None, None, 0) in (0, -1)  # the capacity protocol: the required size comes back
    cap = int(total.value)
    inc, op = ah.Out(cap, np.uint32, True), ah.Out(cap, np.uint8, True)
    assert call(inc.ptr, op.ptr, cap) == 0, lib.zsw_last_error_string(h).decode()
    torch.cuda.synchronize()
    t = int(total.value)
    return {"aln": out.data(), "status": res["status"], "inc": inc.data()[:t], "op": op.data()[:t]}, stats.data()


@pytest.mark.parametrize("annotate", [False, True], ids=["plain", "verbose+NM"])
def test_end_to_end_strands(env, mixed, annotate):
    import torch

    rs, names, quals = mixed
    lib, h = env["lib"], env["h"]
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    reads = [r if i % 2 == 0 else r.translate(comp)[::-1] for i, r in enumerate(rs.reads)]  # every other read from the reverse strand
    rs2 = ah.ReadSet("sam-strands", env["ref"], reads, 0, rs.cls, rs.origin)
    p = ah.Presented(env["_lib"], rs2, "device-ragged")
    n = rs2.n
    o = {k: ah.Out(n, ah.DTYPES[k], True) for k in ("aln", "status", "tier")}
    strand = ah.Out(n, np.uint8, True)
    cap = 16 * n + 64
    inc, op = ah.Out(cap, np.uint32, True), ah.Out(cap, np.uint8, True)
    total = C.c_uint64(0)
    assert lib.zsw_align_3pass_strands_batch_from(h, p.ref(), 8, 256, 0, o["aln"].ptr, o["status"].ptr, o["tier"].ptr, strand.ptr, inc.ptr, op.ptr, cap,
                                                  C.byref(total), None) == 0, lib.zsw_last_error_string(h).decode()
    oriented = ah.Out(len(rs2.bases), np.uint8, True)
    assert lib.zsw_orient_batch(h, p.ref(), strand.ptr, oriented.ptr, None) == 0
    torch.cuda.synchronize()
    t = int(total.value)
    st = strand.data()
    assert 0.25 < st.mean() < 0.6
    res = {"aln": o["aln"].data(), "status": o["status"].data(), "inc": inc.data()[:t], "op": op.data()[:t]}
    flat, off = oriented.data().tobytes(), rs2.offsets
    as_aligned = [flat[int(off[i]):int(off[i + 1])] for i in range(n)]
    plain = [i for i in np.nonzero(st)[0] if set(reads[i]) <= set(b"ACGTNacgtn")][:20]  # (the library's table also complements IUPAC codes)
    assert len(plain) == 20 and all(as_aligned[i] == reads[i].translate(comp)[::-1] for i in plain)
    stats = None
    if annotate:
        res, stats = annotated(env, as_aligned, res)
    b = Batch(as_aligned, res["aln"], res["status"], res["inc"], res["op"], names, quals, st, stats, rname=b"synthref")
    got = check(env, b, "device-ragged")
    lines = got[0].split(b"\n")
    for i in range(n):  # FLAG and the QUAL reversal against `strand`
        f = lines[i].split(b"\t")
        assert f[1] == (b"4" if res["status"][i] != 0 else b"16" if st[i] else b"0"), i
        assert f[10] == (b"*" if not reads[i] else quals[i][::-1] if st[i] else quals[i]), i
        assert f[9] == (as_aligned[i] or b"*"), i


# ---- stream order --------------------------------------------------------------------------------------------------------------

def test_alignment_then_sam_on_one_stream_without_a_host_synchronise(env, mixed):
    import torch

    rs, names, quals = mixed
    lib, h = env["lib"], env["h"]
    want = aligned(env, rs, "zsw_align_3pass_batch_from")
    b = Batch(rs.reads, want["aln"], want["status"], want["inc"], want["op"], names, quals, rname=b"synthref")
    text, off, _ = b.expected()
    stream = torch.cuda.Stream()
    n, t = rs.n, len(want["inc"])
    o = {k: ah.Out(n, ah.DTYPES[k], True) for k in ("aln", "status", "tier")}
    inc, op = ah.Out(t, np.uint32, True), ah.Out(t, np.uint8, True)
    s = Sam(env, b, "device-ragged", stream=stream, device_records=[o["aln"].ptr, o["status"].ptr, inc.ptr, op.ptr])
    buf_ptr, fetch = s.buffer(len(text) + TAIL)
    offs = ah.Out(n + 1, np.uint64, True)
    torch.cuda.synchronize()
    total = C.c_uint64(0)
    assert lib.zsw_align_3pass_batch_from(h, s.p.ref(), 8, 256, 0, o["aln"].ptr, o["status"].ptr, o["tier"].ptr, inc.ptr, op.ptr, t, C.byref(total),
                                          ah.stream_ptr(stream)) == 0
    assert s.call(buf_ptr, len(text), offs.ptr) == 0, s.msg()  # no host synchronise in between
    stream.synchronize()
    got = fetch()
    assert got[: len(text)].tobytes() == text and (got[len(text):] == SENTINEL).all()
    assert np.array_equal(offs.data(), off)


# ---- argument errors -----------------------------------------------------------------------------------------------------------

def test_argument_errors_write_nothing(env):
    _lib, lib, h = env["_lib"], env["lib"], env["h"]
    cases = [c for c in sc.shape_cases(LDS_LINE) if len(c["read"]) == 37][:40]
    b = batch_of(cases, sc.CONFIGS[0], fixed_len=37)
    total = len(b.expected()[0])
    for pres in ("device-fixed", "host-fixed"):
        s = Sam(env, b, pres)
        ptr, fetch = s.buffer(total + TAIL)
        offs = ah.Out(b.n + 1, np.uint64, s.p.device)

        def fields(**kw):
            f = _lib.ZswSamFields()
            for name, _ in f._fields_:
                setattr(f, name, kw.get(name, getattr(s.f, name)))
            return f

        def refused(rc_want, word, **kw):
            s.total.value, s.n_bad.value = 12345, 678
            rc = s.call(ptr, total, offs.ptr, **kw)
            assert rc == rc_want and word in s.msg(), (pres, rc, s.msg())
            s.sync()
            assert (fetch() == SENTINEL).all() and offs.untouched() and s.total.value == 12345 and s.n_bad.value == 678, (pres, word)

        refused(-1, "flag", flags=2)
        refused(-1, "mapq", fields=fields(mapq=256))
        refused(-1, "rname", fields=fields(rname_len=0))
        refused(-1, "rname", fields=fields(rname=b"x" * 256, rname_len=256))
        refused(-1, "null", recs=[None] + s.rec_ptrs[1:])
        refused(-1, "overlaps", fields=fields(quals=ptr + 5))  # out_text over the qualities
        packed = ah.Presented(_lib, s.p.rs, "host-packed4", lib, h, env["m"].mapping.index_map)
        keep, s.p = s.p, packed
        refused(-4, "ZSW_ENCODING_BYTES")
        s.p = keep
        if pres.startswith("host"):
            noff = np.zeros(b.n + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in b.names], out=noff[1:])
            noff[5], noff[6] = noff[6], noff[5]
            assert noff[6] < noff[5]
            refused(-1, "qname_offsets", fields=fields(qname_offsets=noff.ctypes.data))
        assert s.run()[0] == b.expected()[0]  # and the call still works
    assert lib.zsw_sam_batch(None, s.p.ref(), C.byref(s.f), 0, None, None, None, None, 0, None, 0, C.byref(s.total), None, C.byref(s.n_bad), None) == -5


def test_device_names_that_end_in_front_of_their_start_are_empty(env):
    cases = sc.shape_cases(LDS_LINE)[:20]
    b = batch_of(cases, sc.CONFIGS[0])
    s = Sam(env, b, "device-ragged")
    noff = np.zeros(b.n + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in b.names], out=noff[1:])
    noff[8], noff[9] = noff[9], noff[8]  # name 8 ends in front of its start; 7 and 9 change their lengths
    ptr, keep = place(noff, True)
    s.f.qname_offsets = ptr
    flat = b"".join(b.names)
    b.names = [flat[int(noff[i]):int(noff[i + 1])] if noff[i + 1] > noff[i] else b"" for i in range(b.n)]
    assert b.names[8] == b""
    text, off, _ = b.expected()
    got = s.run()
    assert got[0] == text and np.array_equal(got[1], off)


# ---- the Python and C++ layers ---------------------------------------------------------------------------------------------------

def fastq_records(env, n=200, length=100):
    from zoe_amd import synth
    from zoe_amd.records import FastQ

    ref = synth.reference_host(1200)
    reads = synth.reads_host(ref, 4242, n, length)
    reads[3] = ord("N")
    recs = [FastQ("read%d extra" % i, r.tobytes(), bytes(33 + (i + k) % 40 for k in range(length))) for i, r in enumerate(reads)]
    return ref, recs


@pytest.mark.parametrize("opts", [{}, {"three_pass": True}, {"three_pass": True, "nm": True, "verbose_cigar": True}], ids=["plain", "3pass", "3pass-nm-verbose"])
def test_python_layers_equal_the_host_formatting(env, opts):
    from zoe_amd import records

    ref, recs = fastq_records(env)
    m = env["m"]
    want = ("\n".join(str(r) for r in records.align_fastq_to_sam(recs, ref, "synthref", m, GO, GE, **opts)) + "\n").encode()
    assert want.count(b"\t4\t*\t0\t0\t") >= 1 and want.count(b"AS:i:") > 150
    assert records.align_fastq_to_sam_text(recs, ref, "synthref", m, GO, GE, **opts) == want
    if not opts:
        za = env["za"]
        profiles = za.into_local_profile(records.batch_from_fastq(recs), m, GO, GE)
        aln = profiles.sw_align_from_i8(za.SeqSrc.Reference(ref))
        qnames = [r.header.split()[0] for r in recs]
        assert profiles.to_sam_text(aln, qnames, [r.quality for r in recs], "synthref") == want
        text, off = profiles.to_sam_text(aln, qnames, [r.quality for r in recs], "synthref", device=True)
        assert text.is_cuda and text.cpu().numpy().tobytes() == want
        lines = want.split(b"\n")[:-1]
        assert off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(l) + 1 for l in lines])]).tolist()
        bare = profiles.to_sam_text(aln, None, None, "synthref", omit_seq=True).split(b"\n")[0].split(b"\t")
        assert bare[0] == b"*" and bare[9:11] == [b"*", b"*"]


@pytest.mark.parametrize("opts", [["--3pass"], ["--both-strands"], ["--3pass", "--nm", "--verbose-cigar"], ["--3pass", "--min-score", "200"], []],
                         ids=["3pass", "both-strands", "3pass-nm-verbose", "3pass-min-score", "default"])
def test_driver_device_sam_prints_what_the_host_loop_prints(env, tmp_path, opts):
    from zoe_amd import build

    exe = build.build_driver()
    ref, recs = fastq_records(env)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    (tmp_path / "ref.fa").write_bytes(b">synthref test\n" + ref[:600] + b"\n" + ref[600:] + b"\n")
    with open(tmp_path / "reads.fq", "wb") as f:
        for i, r in enumerate(recs):  # every third read from the reverse strand
            seq, qual = (r.sequence.translate(comp)[::-1], r.quality[::-1]) if i % 3 == 1 else (r.sequence, r.quality)
            f.write(b"@" + r.header.encode() + b"\n" + seq + b"\n+\n" + qual + b"\n")
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(__import__("torch").__file__), "lib") + ":" + e.get("LD_LIBRARY_PATH", "")
    run = lambda extra: subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), *opts, *extra], capture_output=True, env=e, timeout=300)
    host, dev = run([]), run(["--device-sam"])
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr, dev.stderr)
    assert host.stdout.startswith(b"@HD\tVN:1.6\n@SQ\tSN:synthref\tLN:1200\n") and host.stdout.count(b"\n") == 202
    assert dev.stdout == host.stdout
    body = host.stdout.split(b"\n")[2:-1]
    if "--both-strands" in opts:
        assert sum(l.split(b"\t")[1] == b"16" for l in body) > 40
    if "--min-score" in opts or not opts or opts == ["--3pass"]:
        assert any(l.split(b"\t")[1] == b"4" for l in body)
