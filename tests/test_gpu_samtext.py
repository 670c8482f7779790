"""GPU tests of zsw_sam_parse_batch through ctypes and the C ABI: every output array and all thirteen report words against the mirror of
the reference's SAM reader (zoe_amd/records.py through tests/samtext_cases.py; clean in the host model first,
tests/test_samtext_model.py).

Every call gets output arrays of exactly the sizes the expectation has, between canary entries, and a report pre-filled with a
pattern. Shapes are the smallest at which the kernels can go wrong: the case list in device and host memory under every flag set;
texts of 0, 1, 15, 16, 17 bytes and one byte either side of a tile; the text at device addresses base + 1, 3, 15; one block of lines
+- 1 and 3,000 mixed lines; a buffer cut at every byte of its last two lines without FINAL, and the chunked restart; a text with more
newlines than the workspace estimate as the first call of a new context; FASTQ and SAM calls in turn on one context (they share the
newline index's workspace); the capacity protocol; NULL outputs; two runs; the argument
errors; a non-default stream; the identities against zsw_sam_batch, zsw_pileup_batch and zsw_annotate_batch; the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_helpers as ah
import samtext_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"FQ_TILE = (\d+);", open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_fastq.hpp")).read()).group(1))
BLOCK_LINES = int(re.search(r"SAM_BLOCK_LINES = (\d+);", open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_samtext.hpp")).read()).group(1))
GO, GE = -10, -1
WORDS = 13
PATTERN = 0xA5A5A5A5
STATS_DTYPE = np.dtype([("matches", "<u4"), ("mismatches", "<u4"), ("ins_bases", "<u4"), ("del_bases", "<u4"), ("ins_runs", "<u4"), ("del_runs", "<u4"),
                        ("path_score", "<i4"), ("path_status", "<u4")])
PARSED_DTYPE = np.dtype([("pos", "<u8"), ("line", "<u8"), ("flag", "<u2"), ("mapq", "u1"), ("code", "u1"), ("bits", "<u4")])
ARRAYS = ("bases", "quals", "offsets", "qnames", "qname_offsets", "aln", "status", "inc", "op", "strand", "parsed")
OPTIONAL = ("quals", "qnames", "strand", "parsed")


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib, synth

    lib = _lib.load()
    assert hasattr(lib, "zsw_sam_parse_batch")
    m = zoe_amd.WeightMatrix.new(zoe_amd.DNA_PROFILE_MAP, 2, -5, b"N")
    ref = synth.reference_host(2000)
    h = ah.new_context(_lib, lib, m, GO, GE, ref)
    yield {"za": zoe_amd, "_lib": _lib, "lib": lib, "m": m, "ref": ref, "h": h}
    lib.zsw_destroy(h)


def test_the_constants_the_shapes_are_built_from():
    assert TILE == 4096 and BLOCK_LINES == 4


class Text:
    """the bytes of a call, in device memory at base + shift or in host memory"""

    def __init__(self, text: bytes, device: bool, shift: int = 0):
        self.n, self.device = len(text), device
        a = np.full(shift + len(text) + 1, 0x0A, dtype=np.uint8)  # newlines in front of and behind the text: a load outside it is counted
        a[shift:shift + len(text)] = np.frombuffer(text, dtype=np.uint8)
        if device:
            import torch

            self.keep = torch.from_numpy(a).cuda()
            assert self.keep.data_ptr() % 256 == 0
            self.ptr = self.keep.data_ptr() + shift
        else:
            self.keep = a
            self.ptr = a.ctypes.data + shift


class Parse:
    """one zsw_sam_parse_batch call with output arrays of the given capacities between canary entries"""

    def __init__(self, env, text: Text, flags, base_cap, name_cap, ciglet_cap, record_cap, rname=None, ref_len=0, without=(), stream=None):
        self.env, self.text, self.flags, self.rname, self.ref_len, self.stream = env, text, flags, rname, ref_len, stream
        dev = text.device
        self.caps = (base_cap, name_cap, ciglet_cap, record_cap)
        shapes = {"bases": (base_cap, np.uint8), "quals": (base_cap, np.uint8), "offsets": (record_cap + 1, np.uint64), "qnames": (name_cap, np.uint8),
                  "qname_offsets": (record_cap + 1, np.uint64), "aln": (record_cap, ah.ALN_DTYPE), "status": (record_cap, np.uint8), "inc": (ciglet_cap, np.uint32),
                  "op": (ciglet_cap, np.uint8), "strand": (record_cap, np.uint8), "parsed": (record_cap, PARSED_DTYPE)}
        skip = set(without) | ({"qname_offsets"} if "qnames" in without else set())
        self.o = {k: ah.Out(n, dt, dev) for k, (n, dt) in shapes.items() if k not in skip}
        self.info = (C.c_uint64 * WORDS)(*([PATTERN] * WORDS))

    def outs(self):
        return list(self.o.values())

    def struct(self, caps=None, **ptrs):
        s = self.env["_lib"].ZswSamParseOut()
        for k, out in self.o.items():
            setattr(s, k, out.ptr)
        s.base_cap, s.name_cap, s.ciglet_cap, s.record_cap = self.caps if caps is None else caps
        for k, v in ptrs.items():
            setattr(s, k, v)
        return s

    def call(self, caps=None, **ptrs):
        env, t = self.env, self.text
        s = self.struct(caps, **ptrs)
        return env["lib"].zsw_sam_parse_batch(env["h"], t.ptr, t.n, env["_lib"].MEM_DEVICE if t.device else env["_lib"].MEM_HOST, self.flags, self.rname,
                                              len(self.rname) if self.rname else 0, self.ref_len, C.byref(s), self.info, ah.stream_ptr(self.stream))

    def msg(self):
        return self.env["lib"].zsw_last_error_string(self.env["h"]).decode()

    def report(self):
        return [int(x) for x in self.info]

    def compare(self, want, tag, exact=True):
        """the arrays against the expectation's; exact: the capacities are the totals, else the arrays are longer and FILL behind them"""
        assert all(o.guards_intact() for o in self.outs()), tag
        for k, w in want.items():
            if k not in self.o:
                continue
            got = self.o[k].data()
            w = np.frombuffer(w, dtype=np.uint8) if isinstance(w, bytes) else w
            assert exact is False or len(got) == len(w), (tag, k)
            assert np.array_equal(got[:len(w)], w.astype(got.dtype) if got.dtype.names is None else w), (tag, k, got[:len(w)][:8], w[:8])
            assert (got[len(w):].view(np.uint8) == ah.FILL).all(), (tag, k)  # nothing behind the totals


def check(env, text: bytes, flags=sc.FINAL, device=True, shift=0, rname=None, ref_len=0, what=""):
    """the call with exactly the capacities the expectation needs -> the expectation"""
    e = sc.Expect(text, flags, rname, ref_len)
    i = e.info
    p = Parse(env, Text(text, device, shift), flags, i[2], i[3], i[4], i[0], rname, ref_len)
    rc = p.call()
    tag = (what, flags, device, shift, rname)
    assert rc == 0, (tag, rc, p.msg())
    assert p.report() == e.info, (tag, dict(zip(sc.INFO, p.report())), dict(zip(sc.INFO, e.info)))
    p.compare(e.arrays(), tag)
    return e


# ---- the case list -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("flags", sc.FLAG_SETS)
def test_the_case_list(env, device, flags):
    rname = b"chr" if flags & sc.QUAL_FORWARD else None
    for name, text in sc.CASES:
        check(env, text, flags, device, rname=rname, ref_len=77, what=name)


# ---- word and tile edges -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    text = sc.mixed_file(40, seed=3)
    assert len(text) > 2 * TILE + 17
    return text


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1])
def test_text_lengths_at_the_word_and_tile_edges(env, big, n):
    for flags in (sc.FINAL, 0):
        for device in (True, False):
            check(env, big[:n], flags, device, what=f"cut{n}")


@pytest.mark.parametrize("shift", [1, 3, 15])
def test_the_text_at_unaligned_device_addresses(env, big, shift):
    for n in (17, TILE - shift, TILE - shift + 1, len(big)):
        check(env, big[:n], sc.FINAL, True, shift, what=f"shift{shift} cut{n}")
    check(env, dict(sc.CASES)["code6_at2"], sc.FINAL, True, shift)
    check(env, dict(sc.CASES)["cigar_run_across_sweep"] + dict(sc.CASES)["opt_lengths"], sc.FINAL | sc.QUAL_FORWARD, True, shift, rname=b"chr")


def test_a_tab_a_newline_and_an_op_either_side_of_a_tile_edge(env):
    special = sc.line(qname=b"edge", cigar=b"3M2I" * 8, seq=sc.seq_of(40))
    g, base_len = sc.good(0), len(sc.line(qname=b""))
    for what, off in (("tab", special.index(b"\t")), ("newline", len(special) - 1), ("op", special.index(b"3M2I") + 1)):
        for at in (TILE - 1, TILE):
            k = (at - off - base_len - 1) // len(g)
            text = sc.line(qname=b"p" * (at - off - base_len - k * len(g))) + g * k + special + g * 2
            assert text[at] == special[off]
            check(env, text, sc.FINAL, True, what=f"{what} at {at}")


# ---- line counts -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, BLOCK_LINES - 1, BLOCK_LINES, BLOCK_LINES + 1])
def test_one_block_of_lines(env, n):
    e = check(env, b"".join(sc.good(i) for i in range(n)), sc.FINAL, True, what=f"n{n}")
    assert e.info[0] == n and e.info[6] == 0


def test_three_thousand_mixed_lines(env):
    text = sc.mixed_file(3000, seed=7, rnames=(b"chr", b"chr", b"chr2"))
    e = check(env, text, sc.FINAL | sc.QUAL_FORWARD, True, rname=b"chr", ref_len=2000, what="3000")
    assert e.info[0] + e.info[1] == 3001 and e.info[1] > 100 and 1000 < e.info[9] < e.info[0] and e.info[11:] == [1, 400]
    assert max(len(r["ciglets"]) for r in e.recs) == 40 and any(r["parsed"][5] & sc.BIT_OTHER_RNAME for r in e.recs)


def test_the_lowest_failing_line_of_many(env):
    parts = [sc.good(i % 5) for i in range(3000)]
    for i in (2999, 2500, 1777, 1778):
        parts[i] = sc.FAULTS[1 + i % 6]
    e = check(env, b"".join(parts), sc.FINAL, True)
    assert e.info[6:8] == [1 + 1777 % 6, 1777] and len(e.recs) == 1777


# ---- without FINAL -----------------------------------------------------------------------------------------------------------

def test_without_final_a_buffer_cut_at_every_byte_of_its_last_two_lines(env):
    text = sc.mixed_file(6, seed=5, max_read=40) + sc.good(2).replace(b"\n", b"\r\n") + sc.good(3)
    ends = [i for i, c in enumerate(text) if c == 10]
    whole = sc.Expect(text).recs
    more = sc.good(4)
    for n in range(ends[-3] + 1, len(text) + 1):
        e = check(env, text[:n], 0, True, what=f"cut{n}")
        full = sum(1 for i in ends if i < n)
        assert e.info[5] == ends[full - 1] + 1 and e.info[6] == 0
        # the rest together with the next chunk gives the remaining records
        rest = check(env, text[e.info[5]:] + more, sc.FINAL, True, what=f"restart{n}")
        strip = lambda recs: [(r["name"], r["bases"], r["quals"], r["status"], r["aln"][:8], r["ciglets"], r["strand"], r["parsed"][0], r["parsed"][2:]) for r in recs]
        assert strip(e.recs) + strip(rest.recs) == strip(whole) + strip(sc.Expect(more).recs)


# ---- the capacity protocol ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_capacity_protocol(env, device):
    text = sc.mixed_file(40, seed=9, max_read=90)
    e = sc.Expect(text)
    nr, nb, nn, nc = e.info[0], e.info[2], e.info[3], e.info[4]
    t = Text(text, device)
    info = (C.c_uint64 * WORDS)()
    mem = env["_lib"].MEM_DEVICE if device else env["_lib"].MEM_HOST
    empty = env["_lib"].ZswSamParseOut()
    assert env["lib"].zsw_sam_parse_batch(env["h"], t.ptr, t.n, mem, sc.FINAL, None, 0, 0, C.byref(empty), info, None) == 0  # the sizing call
    assert [int(x) for x in info] == e.info
    for caps in ((nb - 1, nn, nc, nr), (nb, nn - 1, nc, nr), (nb, nn, nc - 1, nr), (nb, nn, nc, nr - 1), (0, 0, 0, 0)):
        p = Parse(env, t, sc.FINAL, nb, nn, nc, nr)
        assert p.call(caps) == -1 and "capacity" in p.msg(), caps
        assert p.report() == e.info, caps  # the needed sizes
        assert all(o.untouched() for o in p.outs()), caps
    p = Parse(env, t, sc.FINAL, nb, nn - 1, nc, nr, without=("qnames",))  # without names their capacity does not matter
    assert p.call() == 0 and p.report() == e.info
    p.compare(e.arrays(), "no names")


@pytest.mark.parametrize("text", [b"\t0\t\t0\t0\t\t\t\t\t\t", (b"\t0\t\t0\t0\t\t\t\t\t\t\n") * 9, sc.line(qname=b"n" * 50, cigar=b"1M" * 30, seq=sc.seq_of(30)), b"\n" * 100,
                                  b"@x\n" * 50, sc.five({})], ids=["one", "nine", "ciglets", "newlines", "headers", "five"])
def test_the_stated_upper_bounds_suffice(env, text):
    n = len(text)
    e = sc.Expect(text)
    p = Parse(env, Text(text, True), sc.FINAL, n, n, n // 2, n // 14 + 1)
    assert p.call() == 0, p.msg()
    assert p.report() == e.info
    p.compare(e.arrays(), "bounds", exact=False)


DENSE = [b"@x\n" * 2000, sc.five({}) + b"@\n" * 3000]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("text", DENSE, ids=["headers", "lines_then_headers"])
def test_a_text_denser_than_the_workspace_estimate_on_a_new_context(env, text, device):
    """The workspace of a context only grows, so the repeat of the launches after an overflow of the newline positions runs only
    where a dense text is the first call of a context: more newlines than the n / 64 + 64 positions the entry point provides."""
    assert text.count(b"\n") > len(text) // 64 + 64 + 4
    fresh = dict(env, h=ah.new_context(env["_lib"], env["lib"], env["m"], GO, GE, None))
    try:
        for flags in (sc.FINAL, 0):  # the first call overflows and repeats; the second finds the larger workspace
            check(fresh, text, flags, device, what="dense first")
        check(fresh, sc.mixed_file(40, seed=11), sc.FINAL | sc.QUAL_FORWARD, device, what="normal after dense")
        check(fresh, text[:len(text) // 2], sc.FINAL, device, shift=3 if device else 0, what="dense again")
    finally:
        env["lib"].zsw_destroy(fresh["h"])


def fastq_call(env, text: bytes, device):
    """zsw_fastq_parse_batch with exactly the capacities the expectation needs, checked as tests/test_gpu_fastq.py checks its
    case list -> (the report, the arrays' bytes)"""
    import fastq_cases as fc

    recs, want_info, _ = fc.expect(text, fc.FINAL)
    want = fc.arrays(recs)  # bases, qualities, offsets, names, name offsets
    t = Text(text, device)
    outs = [ah.Out(len(w), np.uint8 if isinstance(w, bytes) else np.uint64, device) for w in want]
    info = (C.c_uint64 * 9)(*([PATTERN] * 9))
    rc = env["lib"].zsw_fastq_parse_batch(env["h"], t.ptr, t.n, env["_lib"].MEM_DEVICE if device else env["_lib"].MEM_HOST, fc.FINAL, outs[0].ptr, outs[1].ptr,
                                          len(want[0]), outs[2].ptr, outs[3].ptr, len(want[3]), outs[4].ptr, len(recs), info, None)
    assert rc == 0, env["lib"].zsw_last_error_string(env["h"]).decode()
    assert [int(x) for x in info] == want_info
    assert all(o.guards_intact() for o in outs)
    got = [o.data() for o in outs]
    for g, w in zip(got, want):
        assert (g.tobytes() == w) if isinstance(w, bytes) else np.array_equal(g, w)
    return [int(x) for x in info], [g.tobytes() for g in got]


def sam_call(env, text: bytes, device):
    """check() -> (the report, the arrays' bytes)"""
    e = sc.Expect(text, sc.FINAL)
    i = e.info
    p = Parse(env, Text(text, device), sc.FINAL, i[2], i[3], i[4], i[0])
    assert p.call() == 0, p.msg()
    assert p.report() == e.info, (dict(zip(sc.INFO, p.report())), dict(zip(sc.INFO, e.info)))
    p.compare(e.arrays(), "shared index")
    return p.report(), [o.data().tobytes() for o in p.outs()]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_fastq_and_sam_calls_share_the_index_workspace_of_one_context(env, device):
    """The two parse calls keep the staged text, the tile counts and the newline positions in one workspace of the context. A FASTQ
    text of one tile and a byte, the dense SAM text (its second round grows the positions under the FASTQ call's sizes), the FASTQ
    text again and a SAM text of one line, on one context: every call gives what it gives as the only call of a new context."""
    import fastq_cases as fc

    fastq = fc.mixed_file(60, 1, 400, seed=3)[:TILE + 1]
    assert len(fastq) == TILE + 1 and DENSE[0].count(b"\n") > 2 * ((TILE + 1) // 16 + 64)  # more than the FASTQ call's positions and their slack
    steps = [(fastq_call, fastq), (sam_call, DENSE[0]), (fastq_call, fastq), (sam_call, sc.good(0))]
    new = lambda: dict(env, h=ah.new_context(env["_lib"], env["lib"], env["m"], GO, GE, None))
    shared = new()
    try:
        for k, (call, text) in enumerate(steps):
            got = call(shared, text, device)
            fresh = new()
            try:
                assert got == call(fresh, text, device), k
            finally:
                env["lib"].zsw_destroy(fresh["h"])
    finally:
        env["lib"].zsw_destroy(shared["h"])


# ---- NULL outputs, determinism, argument errors, streams ---------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_each_optional_output_null_in_turn(env, device):
    text = sc.mixed_file(20, seed=2, max_read=70)
    e = sc.Expect(text, sc.FINAL | sc.QUAL_FORWARD)
    i = e.info
    for without in [(k,) for k in OPTIONAL] + [OPTIONAL]:
        p = Parse(env, Text(text, device), sc.FINAL | sc.QUAL_FORWARD, i[2], i[3], i[4], i[0], without=without)
        assert p.call() == 0, (without, p.msg())
        assert p.report() == e.info
        p.compare(e.arrays(), without)


def test_two_calls_give_identical_arrays(env):
    parts = [sc.good(i % 5) for i in range(2000)]
    for i in range(1500, 2000, 7):  # many failing lines: the lowest one is the same every time
        parts[i] = sc.FAULTS[1 + i % 6]
    text = b"".join(parts)
    n = len(text)
    runs = []
    for _ in range(2):
        p = Parse(env, Text(text, True), sc.FINAL, n, n, n // 2, n // 14 + 1)
        assert p.call() == 0
        runs.append((p.report(), [o.fetch().tobytes() for o in p.outs()]))
    assert runs[0] == runs[1] and runs[0][0][6:8] == [1 + 1500 % 6, 1500]


def test_argument_errors_write_nothing(env):
    _lib, lib, h = env["_lib"], env["lib"], env["h"]
    text = sc.mixed_file(6, seed=4, max_read=30)
    t = Text(text, True)
    n = len(text)
    caps = (n, n, n // 2, n // 14 + 1)

    def call(p, h=h, text_ptr=t.ptr, n_bytes=n, mem=_lib.MEM_DEVICE, flags=sc.FINAL, rname=None, rname_len=0, info="own", out="own", **ptrs):
        s = p.struct(**ptrs)
        return lib.zsw_sam_parse_batch(h, text_ptr, n_bytes, mem, flags, rname, rname_len, 0, C.byref(s) if out == "own" else None, p.info if info == "own" else None, None)

    p = Parse(env, t, sc.FINAL, *caps)
    o = p.o
    bad = [dict(h=None), dict(info=None), dict(out=None), dict(text_ptr=None), dict(flags=4), dict(flags=sc.FINAL | 8), dict(mem=7), dict(rname=b"chr", rname_len=0),
           dict(rname=None, rname_len=3), dict(rname=b"c" * 300, rname_len=300), dict(bases=None), dict(offsets=None), dict(aln=None), dict(status=None), dict(inc=None),
           dict(op=None), dict(qnames=None), dict(qname_offsets=None), dict(quals=o["bases"].ptr), dict(qnames=o["bases"].ptr + 1), dict(bases=t.ptr + 3),
           dict(offsets=t.ptr), dict(qname_offsets=o["offsets"].ptr + 8), dict(qnames=t.ptr + n - 1), dict(inc=o["aln"].ptr), dict(op=o["status"].ptr),
           dict(strand=o["status"].ptr), dict(parsed=o["aln"].ptr + 8), dict(status=t.ptr + 1)]
    for kw in bad:
        assert call(p, **kw) == -1, kw
        assert all(x.untouched() for x in p.outs()) and p.report() == [PATTERN] * WORDS, kw
    assert call(p, text_ptr=None, n_bytes=0) == 0 and p.report() == [0] * WORDS  # no text is needed for no bytes
    q = Parse(env, t, sc.FINAL, *caps)
    assert call(q) == 0 and q.report() == sc.Expect(text).info


def test_a_call_on_a_non_default_stream(env):
    import torch

    text = sc.mixed_file(200, seed=21, max_read=150)
    e = sc.Expect(text, sc.FINAL, b"chr", 9)
    stream = torch.cuda.Stream()
    i = e.info
    p = Parse(env, Text(text, True), sc.FINAL, i[2], i[3], i[4], i[0], b"chr", 9, stream=stream)
    torch.cuda.synchronize()
    assert p.call() == 0, p.msg()
    assert p.report() == e.info
    p.compare(e.arrays(), "stream")


# ---- identities against the existing calls -----------------------------------------------------------------------------------

N_READS, READ_LEN = 5000, 150


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, copy=True)).cuda()


def sam_batch(env, batch, fields, aln, status, inc, op, n_ciglets):
    """zsw_sam_batch over device arrays -> the text as a CUDA tensor"""
    import torch

    lib, h = env["lib"], env["h"]
    total, n_bad = C.c_uint64(0), C.c_uint64(0)
    args = (h, C.byref(batch), C.byref(fields), 0, aln, status, inc, op, n_ciglets)
    assert lib.zsw_sam_batch(*args, None, 0, C.byref(total), None, C.byref(n_bad), None) == 0, lib.zsw_last_error_string(h).decode()
    text = torch.empty(int(total.value), dtype=torch.uint8, device="cuda")
    assert lib.zsw_sam_batch(*args, text.data_ptr(), int(total.value), C.byref(total), None, C.byref(n_bad), None) == 0
    torch.cuda.synchronize()
    assert n_bad.value == 0
    return text


def parse_device(env, d_text, rname=b"synthref", ref_len=2000):
    """zsw_sam_parse_batch over a CUDA tensor with exactly sized outputs -> (dict of CUDA tensors, report)"""
    import torch

    lib, h, _lib = env["lib"], env["h"], env["_lib"]
    info = (C.c_uint64 * WORDS)()
    o = _lib.ZswSamParseOut()
    head = (h, d_text.data_ptr(), d_text.numel(), _lib.MEM_DEVICE, sc.FINAL | sc.QUAL_FORWARD, rname, len(rname) if rname else 0, ref_len)
    assert lib.zsw_sam_parse_batch(*head, C.byref(o), info, None) == 0
    nr, nb, nn, nc = int(info[0]), int(info[2]), int(info[3]), int(info[4])
    sizes = {"bases": nb, "quals": nb, "offsets": (nr + 1) * 8, "qnames": nn, "qname_offsets": (nr + 1) * 8, "aln": nr * 40, "status": nr, "inc": nc * 4, "op": nc,
             "strand": nr, "parsed": nr * 24}
    t = {k: torch.empty(max(v, 1), dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    for k, v in t.items():
        setattr(o, k, v.data_ptr())
    o.base_cap, o.name_cap, o.ciglet_cap, o.record_cap = nb, nn, nc, nr
    assert lib.zsw_sam_parse_batch(*head, C.byref(o), info, None) == 0, lib.zsw_last_error_string(h).decode()
    return {k: v[:sizes[k]] for k, v in t.items()}, [int(x) for x in info]


@pytest.fixture(scope="module")
def aligned(env):
    """5,000 synthetic reads, every other one from the reverse strand, through zsw_align_3pass_strands_batch_from and zsw_sam_batch"""
    import torch

    from zoe_amd import synth

    lib, h, _lib = env["lib"], env["h"], env["_lib"]
    reads = synth.reads_host(env["ref"], 31000, N_READS, READ_LEN).reshape(N_READS, READ_LEN).copy()
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    reads[1::2] = comp[reads[1::2, ::-1]]
    reads[7] = ord("N")  # one read without an alignment
    d_reads = dev(reads.reshape(-1))
    b = _lib.ZswBatch()
    b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem, b.encoding = d_reads.data_ptr(), None, READ_LEN, N_READS, _lib.MEM_DEVICE, 0
    d_aln = torch.zeros(N_READS * 40, dtype=torch.uint8, device="cuda")
    d_status, d_tier, d_strand = (torch.zeros(N_READS, dtype=torch.uint8, device="cuda") for _ in range(3))
    cap = 16 * N_READS + 64
    d_inc, d_op = torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.zeros(cap, dtype=torch.uint8, device="cuda")
    total = C.c_uint64(0)
    assert lib.zsw_align_3pass_strands_batch_from(h, C.byref(b), 8, 256, 0, d_aln.data_ptr(), d_status.data_ptr(), d_tier.data_ptr(), d_strand.data_ptr(),
                                                  d_inc.data_ptr(), d_op.data_ptr(), cap, C.byref(total), None) == 0, lib.zsw_last_error_string(h).decode()
    d_oriented = torch.empty_like(d_reads)
    assert lib.zsw_orient_batch(h, C.byref(b), d_strand.data_ptr(), d_oriented.data_ptr(), None) == 0
    torch.cuda.synchronize()
    ob = _lib.ZswBatch()
    ob.bases, ob.offsets, ob.fixed_len, ob.n_reads, ob.mem, ob.encoding = d_oriented.data_ptr(), None, READ_LEN, N_READS, _lib.MEM_DEVICE, 0
    names = [b"read/%d" % i for i in range(N_READS)]
    noff = np.cumsum([0] + [len(x) for x in names]).astype(np.int64)
    rng = np.random.default_rng(3)
    quals = rng.integers(33, 127, N_READS * READ_LEN, dtype=np.uint8)
    d = dict(b=ob, aln=d_aln, status=d_status, strand=d_strand, inc=d_inc, op=d_op, t=int(total.value), oriented=d_oriented, names=dev(np.frombuffer(b"".join(names), np.uint8)),
             noff=dev(noff), quals=dev(quals), h_quals=quals.reshape(N_READS, READ_LEN), h_names=b"".join(names), h_noff=noff)
    f = _lib.ZswSamFields()
    f.qnames, f.qname_offsets, f.quals, f.strand = d["names"].data_ptr(), d["noff"].data_ptr(), d["quals"].data_ptr(), d_strand.data_ptr()
    f.rname, f.rname_len, f.mapq = b"synthref", 8, 255
    d["fields"] = f
    d["text"] = sam_batch(env, ob, f, d_aln.data_ptr(), d_status.data_ptr(), d_inc.data_ptr(), d_op.data_ptr(), d["t"])
    return d


def ciglets_of(aln, inc, op, i):
    o, n = int(aln[i]["ciglet_offset"]), int(aln[i]["n_ciglets"])
    return inc[o:o + n].tolist(), op[o:o + n].tolist()


def test_identity_a_sam_text_parsed_gives_back_the_records(env, aligned):
    d = aligned
    t, info = parse_device(env, d["text"])
    assert info[0] == N_READS and info[1] == 0 and info[6] == 0 and info[10] == 0 and info[5] == d["text"].numel()
    status, strand = d["status"].cpu().numpy(), d["strand"].cpu().numpy()
    aln = d["aln"].cpu().numpy().view(ah.ALN_DTYPE)
    inc, op = d["inc"].cpu().numpy().view(np.uint32), d["op"].cpu().numpy()
    g_aln, g_status, g_strand = t["aln"].cpu().numpy().view(ah.ALN_DTYPE), t["status"].cpu().numpy(), t["strand"].cpu().numpy()
    g_inc, g_op = t["inc"].cpu().numpy().view(np.uint32), t["op"].cpu().numpy()
    some = status == 0
    assert 0.9 * N_READS < some.sum() < N_READS and info[9] == some.sum() and 0.25 < strand.mean() < 0.75
    assert np.array_equal(g_status == 0, some) and (g_status[~some] == 2).all() and not g_aln[~some].view(np.uint8).any()
    for k in ("score", "ref_start", "ref_end", "query_start", "query_end", "ref_len", "query_len", "n_ciglets"):
        assert np.array_equal(g_aln[k][some], aln[k][some]), k
    assert np.array_equal(g_aln["ciglet_offset"][some], np.cumsum(np.concatenate(([0], aln["n_ciglets"][some])))[:-1])  # laid out in record order
    for i in np.nonzero(some)[0]:
        assert ciglets_of(g_aln, g_inc, g_op, i) == ciglets_of(aln, inc, op, i), i
    assert info[4] == int(aln["n_ciglets"][some].sum())
    assert np.array_equal(t["bases"].cpu().numpy(), d["oriented"].cpu().numpy())
    # an unmapped line has FLAG 4: no strand, and zsw_sam_batch wrote its QUAL back to front where the strand array said so
    assert np.array_equal(g_strand, np.where(some, strand, 0))
    want_quals = np.where(((strand != 0) & ~some)[:, None], d["h_quals"][:, ::-1], d["h_quals"])
    assert np.array_equal(t["quals"].cpu().numpy().reshape(N_READS, READ_LEN), want_quals)
    assert t["qnames"].cpu().numpy().tobytes() == d["h_names"] and np.array_equal(t["qname_offsets"].cpu().numpy().view(np.int64), d["h_noff"])
    assert np.array_equal(t["offsets"].cpu().numpy().view(np.int64), np.arange(N_READS + 1) * READ_LEN)
    # a second zsw_sam_batch on the parsed arrays gives the same bytes as the first
    _lib = env["_lib"]
    b = _lib.ZswBatch()
    b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem, b.encoding = t["bases"].data_ptr(), t["offsets"].data_ptr(), 0, N_READS, _lib.MEM_DEVICE, 0
    f = _lib.ZswSamFields()
    f.qnames, f.qname_offsets, f.quals, f.strand = t["qnames"].data_ptr(), t["qname_offsets"].data_ptr(), t["quals"].data_ptr(), d["strand"].data_ptr()
    f.rname, f.rname_len, f.mapq = b"synthref", 8, 255
    again = sam_batch(env, b, f, t["aln"].data_ptr(), t["status"].data_ptr(), t["inc"].data_ptr(), t["op"].data_ptr(), info[4])
    assert again.numel() == d["text"].numel() and bool((again == d["text"]).all())


def pileup_and_annotate(env, b, aln, status, inc, op, n_ciglets):
    import torch

    lib, h = env["lib"], env["h"]
    L = len(env["ref"])
    counts = torch.zeros(L * 8, dtype=torch.int32, device="cuda")
    ins = torch.zeros((L + 1) * 2, dtype=torch.int32, device="cuda")
    stats = torch.zeros(N_READS * 32, dtype=torch.uint8, device="cuda")
    n_bad = C.c_uint64(0)
    assert lib.zsw_pileup_batch(h, C.byref(b), env["_lib"].PILEUP_CLEAR, aln, status, inc, op, n_ciglets, counts.data_ptr(), ins.data_ptr(), C.byref(n_bad), None) == 0, \
        lib.zsw_last_error_string(h).decode()
    assert lib.zsw_annotate_batch(h, C.byref(b), 0, aln, status, inc, op, n_ciglets, stats.data_ptr(), None, None, None, 0, None, None) == 0, lib.zsw_last_error_string(h).decode()
    torch.cuda.synchronize()
    return counts.cpu().numpy(), ins.cpu().numpy(), stats.cpu().numpy().view(STATS_DTYPE), int(n_bad.value)


def parsed_batch(env, t):
    _lib = env["_lib"]
    b = _lib.ZswBatch()
    b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem, b.encoding = t["bases"].data_ptr(), t["offsets"].data_ptr(), 0, N_READS, _lib.MEM_DEVICE, 0
    return b


def test_identity_b_pileup_and_annotate_on_the_parsed_arrays(env, aligned):
    d = aligned
    t, info = parse_device(env, d["text"])
    want = pileup_and_annotate(env, d["b"], d["aln"].data_ptr(), d["status"].data_ptr(), d["inc"].data_ptr(), d["op"].data_ptr(), d["t"])
    got = pileup_and_annotate(env, parsed_batch(env, t), t["aln"].data_ptr(), t["status"].data_ptr(), t["inc"].data_ptr(), t["op"].data_ptr(), info[4])
    assert want[3] == 0 and got[3] == 0 and want[0].sum() > 100 * N_READS
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])  # the whole table
    assert np.array_equal(got[2], want[2])                                     # every stats entry


def test_identity_c_the_verbose_text_parsed_has_the_verbose_ciglets(env, aligned):
    import torch

    d = aligned
    lib, h = env["lib"], env["h"]
    v_aln = torch.zeros(N_READS * 40, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(N_READS * 32, dtype=torch.uint8, device="cuda")
    total = C.c_uint64(0)
    for cap in (0, None):  # the capacity protocol of zsw_annotate_batch: the first call reports the number of verbose ciglets
        cap = int(total.value) if cap is None else cap
        v_inc, v_op = torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda"), torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
        rc = lib.zsw_annotate_batch(h, C.byref(d["b"]), 0, d["aln"].data_ptr(), d["status"].data_ptr(), d["inc"].data_ptr(), d["op"].data_ptr(), d["t"], stats.data_ptr(),
                                    v_aln.data_ptr(), v_inc.data_ptr(), v_op.data_ptr(), cap, C.byref(total), None)
    assert rc == 0 and total.value > d["t"], lib.zsw_last_error_string(h).decode()
    torch.cuda.synchronize()
    text = sam_batch(env, d["b"], d["fields"], v_aln.data_ptr(), d["status"].data_ptr(), v_inc.data_ptr(), v_op.data_ptr(), int(total.value))
    t, info = parse_device(env, text)
    assert info[0] == N_READS and info[6] == 0 and info[10] == 0
    some = d["status"].cpu().numpy() == 0
    aln, inc, op = v_aln.cpu().numpy().view(ah.ALN_DTYPE), v_inc.cpu().numpy().view(np.uint32), v_op.cpu().numpy()
    g_aln, g_inc, g_op = t["aln"].cpu().numpy().view(ah.ALN_DTYPE), t["inc"].cpu().numpy().view(np.uint32), t["op"].cpu().numpy()
    assert info[4] == int(aln["n_ciglets"][some].sum()) and set(g_op.tolist()) >= {ord("="), ord("X")} and ord("M") not in set(g_op.tolist())
    for i in np.nonzero(some)[0]:
        assert ciglets_of(g_aln, g_inc, g_op, i) == ciglets_of(aln, inc, op, i), i


def test_identity_d_a_two_reference_text_piles_up_only_the_named_reference(env, aligned):
    import torch

    d = aligned
    lines = d["text"].cpu().numpy().tobytes().split(b"\n")[:-1]
    other = np.zeros(N_READS, dtype=bool)
    other[::3] = True
    text = b"".join((ln.replace(b"\tsynthref\t", b"\tsynthref2\t", 1) if other[i] else ln) + b"\n" for i, ln in enumerate(lines))
    t, info = parse_device(env, dev(np.frombuffer(text, np.uint8)))
    status = d["status"].cpu().numpy()
    masked = np.where(other, 2, status).astype(np.uint8)
    assert info[0] == N_READS and info[9] == int((masked == 0).sum()) and np.array_equal(t["status"].cpu().numpy(), np.where(masked == 0, 0, 2))
    bits = t["parsed"].cpu().numpy().view(PARSED_DTYPE)["bits"]
    assert np.array_equal((bits & sc.BIT_OTHER_RNAME) != 0, other & (status == 0))
    d_masked = dev(masked)
    want = pileup_and_annotate(env, d["b"], d["aln"].data_ptr(), d_masked.data_ptr(), d["inc"].data_ptr(), d["op"].data_ptr(), d["t"])
    got = pileup_and_annotate(env, parsed_batch(env, t), t["aln"].data_ptr(), t["status"].data_ptr(), t["inc"].data_ptr(), t["op"].data_ptr(), info[4])
    assert got[3] == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    everything, _ = parse_device(env, dev(np.frombuffer(text, np.uint8)), rname=None)  # without rname every mapped line is converted
    assert int((everything["status"].cpu().numpy() == 0).sum()) == int((status == 0).sum())
    torch.cuda.synchronize()


# ---- the Python layer --------------------------------------------------------------------------------------------------------

def test_python_layer_sam_batch_from_text_to_pileup(env, aligned):
    from zoe_amd import SeqSrc, into_local_profile, records

    d = aligned
    text = d["text"].cpu().numpy().tobytes()
    header = b"@HD\tVN:1.6\n@SQ\tSN:synthref\tLN:2000\n"
    sam = records.sam_batch_from_text(header + text, rname="synthref", ref_len=len(env["ref"]))
    assert len(sam) == N_READS and sam.headers == 2 and sam.consumed == len(header) + len(text)
    profiles = into_local_profile(sam.reads, env["m"], GO, GE)
    src = SeqSrc.Reference(env["ref"])
    counts = profiles.pileup(sam.alignments, src).cpu().numpy()
    want = pileup_and_annotate(env, d["b"], d["aln"].data_ptr(), d["status"].data_ptr(), d["inc"].data_ptr(), d["op"].data_ptr(), d["t"])
    assert np.array_equal(counts.reshape(-1), want[0])
    assert np.array_equal(sam.strand, np.where(d["status"].cpu().numpy() == 0, d["strand"].cpu().numpy(), 0))
    original = into_local_profile(sam.original_reads(), env["m"], GO, GE)
    assert original.to_sam_text(sam.alignments, sam.names, sam.quals, "synthref", 255, strands=sam.strand) == text
    with pytest.raises(records.SamError, match="line 3.*mapq") as e:
        records.sam_batch_from_text(header + sc.good(0) + sc.FAULTS[sc.INVALID_MAPQ] + sc.good(1))
    assert e.value.code == sc.INVALID_MAPQ and e.value.line == 3
    empty = records.sam_batch_from_text(b"")
    assert len(empty) == 0 and empty.consumed == 0
