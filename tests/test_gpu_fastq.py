"""GPU tests of zsw_fastq_parse_batch through ctypes and the C ABI: every output array and all nine report words against what
records.FastQReader yields over the same bytes (tests/fastq_cases.py; clean in the host model first, tests/test_fastq_model.py).

Every call gets output arrays of exactly the sizes the expectation has, between canary entries: a byte written past a capacity, or
not written inside it, shows. Shapes are the smallest at which the kernels can go wrong: the case list in device and host memory
under every flag set; texts of 0, 1, 15, 16, 17 bytes and one byte either side of a tile, a newline on either side of a tile
edge, the text at device addresses base + 1, 3, 15; one block of records +- 1 and 3,000 of mixed lengths; a buffer cut at every
byte of its last two records without FINAL, and the chunked restart; the capacity protocol; a text
with more newlines than the workspace estimate as the first call of a new context; NULL outputs; two runs; the argument
errors; parse -> 3-pass alignment -> annotate -> SAM on one stream; the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_helpers as ah
import fastq_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_fastq.hpp")).read()
TILE = int(re.search(r"FQ_TILE = (\d+);", HPP).group(1))
BLOCK_RECORDS = int(re.search(r"FQ_BLOCK_RECORDS = (\d+);", HPP).group(1))
GO, GE = -10, -1
STATS_DTYPE = np.dtype([("matches", "<u4"), ("mismatches", "<u4"), ("ins_bases", "<u4"), ("del_bases", "<u4"), ("ins_runs", "<u4"), ("del_runs", "<u4"),
                        ("path_score", "<i4"), ("path_status", "<u4")])


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib, synth

    lib = _lib.load()
    assert hasattr(lib, "zsw_fastq_parse_batch")
    m = zoe_amd.WeightMatrix.new(zoe_amd.DNA_PROFILE_MAP, 2, -5, b"N")
    ref = synth.reference_host(2000)
    h = ah.new_context(_lib, lib, m, GO, GE, ref)
    yield {"za": zoe_amd, "_lib": _lib, "lib": lib, "m": m, "ref": ref, "h": h}
    lib.zsw_destroy(h)


def test_the_constants_the_shapes_are_built_from():
    assert TILE == 4096 and BLOCK_RECORDS == 8 and int(re.search(r"FQ_G = (\d+);", HPP).group(1)) == 64


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
    """one zsw_fastq_parse_batch call with output arrays of the given capacities between canary entries"""

    def __init__(self, env, text: Text, flags, base_cap, name_cap, record_cap, quals=True, names=True, stream=None):
        self.env, self.text, self.flags, self.stream = env, text, flags, stream
        dev = text.device
        self.caps = (base_cap, name_cap, record_cap)
        self.bases = ah.Out(base_cap, np.uint8, dev)
        self.quals = ah.Out(base_cap, np.uint8, dev) if quals else None
        self.off = ah.Out(record_cap + 1, np.uint64, dev)
        self.names = ah.Out(name_cap, np.uint8, dev) if names else None
        self.noff = ah.Out(record_cap + 1, np.uint64, dev) if names else None
        self.info = (C.c_uint64 * 9)(*([0xA5A5A5A5] * 9))

    def outs(self):
        return [o for o in (self.bases, self.quals, self.off, self.names, self.noff) if o is not None]

    def call(self, caps=None):
        env, t = self.env, self.text
        base_cap, name_cap, record_cap = self.caps if caps is None else caps
        ptr = lambda o: None if o is None else o.ptr
        rc = env["lib"].zsw_fastq_parse_batch(env["h"], t.ptr, t.n, env["_lib"].MEM_DEVICE if t.device else env["_lib"].MEM_HOST, self.flags, self.bases.ptr,
                                              ptr(self.quals), base_cap, self.off.ptr, ptr(self.names), name_cap, ptr(self.noff), record_cap, self.info,
                                              ah.stream_ptr(self.stream))
        return rc

    def msg(self):
        return self.env["lib"].zsw_last_error_string(self.env["h"]).decode()

    def report(self):
        return [int(x) for x in self.info]


def check(env, text: bytes, flags=fc.FINAL, device=True, shift=0, what=""):
    """the call with exactly the capacities the expectation needs -> (records, report)"""
    recs, want_info, _ = fc.expect(text, flags)
    w_bases, w_quals, w_off, w_names, w_noff = fc.arrays(recs)
    p = Parse(env, Text(text, device, shift), flags, len(w_bases), len(w_names), len(recs))
    rc = p.call()
    tag = (what, flags, device, shift)
    assert rc == 0, (tag, rc, p.msg())
    assert p.report() == want_info, (tag, dict(zip(fc.INFO, p.report())), dict(zip(fc.INFO, want_info)))
    assert all(o.guards_intact() for o in p.outs()), tag
    assert p.bases.data().tobytes() == w_bases and p.quals.data().tobytes() == w_quals and p.names.data().tobytes() == w_names, tag
    assert np.array_equal(p.off.data(), w_off) and np.array_equal(p.noff.data(), w_noff), tag
    return recs, want_info


# ---- the case list -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("flags", fc.FLAG_SETS)
def test_the_case_list(env, device, flags):
    for name, text in fc.CASES:
        check(env, text, flags, device, what=name)


# ---- word and tile edges -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    text = fc.mixed_file(60, 1, 400, seed=3)
    assert len(text) > 2 * TILE + 17
    return text


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1])
def test_text_lengths_at_the_word_and_tile_edges(env, big, n):
    for flags in (fc.FINAL, 0):
        for device in (True, False):
            check(env, big[:n], flags, device, what=f"cut{n}")


def test_a_newline_either_side_of_a_tile_edge(env, big):
    ends = [i for i, c in enumerate(big) if c == 10]
    e = next(i for i in ends if i >= TILE)
    last, first = big[e - (TILE - 1):], big[e - TILE:]
    assert last[TILE - 1] == 10 and first[TILE] == 10
    for text in (last, first):
        for flags in (fc.FINAL, 0):
            check(env, text, flags, True, what="tile edge")


@pytest.mark.parametrize("shift", [1, 3, 15])
def test_the_text_at_unaligned_device_addresses(env, big, shift):
    for n in (17, TILE - shift, TILE - shift + 1, len(big)):
        check(env, big[:n], fc.FINAL, True, shift, what=f"shift{shift} cut{n}")
    check(env, dict(fc.CASES)["code8_at2"], fc.FINAL, True, shift)
    check(env, b"".join(t for _, t in fc.CASES[1:6] if t.endswith(b"\n")), 0, True, shift)


# ---- record counts -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, BLOCK_RECORDS - 1, BLOCK_RECORDS, BLOCK_RECORDS + 1, 3000])
def test_record_counts(env, n):
    recs, info = check(env, fc.mixed_file(n, 1, 400, seed=n), fc.FINAL | fc.NAME_TO_BLANK, True, what=f"n{n}")
    assert info[0] == n and info[4] == 0 and (n == 1 or info[7:9] == [1, 400])


def test_the_lowest_failing_record_of_many(env):
    parts = [fc.rec(b"r%d x" % i, fc.seq_of(1 + i % 90, i), fc.qual_of(1 + i % 90, i)) for i in range(3000)]
    for i in (2999, 2500, 1777, 1778):
        parts[i] = fc.FAULTS[1 + i % 8]
    recs, info = check(env, b"".join(parts), fc.FINAL, True)
    assert info[4:6] == [1 + 1777 % 8, 1777] and len(recs) == 1777


# ---- without FINAL -----------------------------------------------------------------------------------------------------------

def test_without_final_a_buffer_cut_at_every_byte_of_its_last_two_records(env):
    text = fc.mixed_file(5, 3, 40, seed=5) + fc.rec(b"crlf one", b"ACGTAC", eol=b"\r\n") + fc.rec(b"last", b"ACG")
    ends = [i for i, c in enumerate(text) if c == 10]
    all_recs = fc.expect(text)[0]
    assert len(all_recs) == 7
    next_chunk = fc.rec(b"next", b"ACGTT")
    for n in range(ends[-9] + 1, len(text) + 1):
        recs, info = check(env, text[:n], 0, True, what=f"cut{n}")
        full = sum(1 for i in ends if i < n) // 4
        assert info[0] == full and info[3] == (ends[4 * full - 1] + 1 if full else 0) and info[4] == 0
        # the rest together with the next chunk gives the remaining records
        rest, _ = check(env, text[info[3]:n] + text[n:] + next_chunk, fc.FINAL, True, what=f"restart{n}")
        assert recs + rest == all_recs + [(b"next", b"ACGTT", b"IIIII")]


# ---- the capacity protocol ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_capacity_protocol(env, device):
    text = fc.mixed_file(40, 1, 90, seed=9)
    recs, want_info, _ = fc.expect(text)
    nb, nn, nr = want_info[1], want_info[2], want_info[0]
    t = Text(text, device)
    info = (C.c_uint64 * 9)()
    mem = env["_lib"].MEM_DEVICE if device else env["_lib"].MEM_HOST
    assert env["lib"].zsw_fastq_parse_batch(env["h"], t.ptr, t.n, mem, fc.FINAL, None, None, 0, None, None, 0, None, 0, info, None) == 0  # the sizing call
    assert [int(x) for x in info] == want_info
    for caps in ((nb - 1, nn, nr), (nb, nn - 1, nr), (nb, nn, nr - 1), (0, 0, 0)):
        p = Parse(env, t, fc.FINAL, nb, nn, nr)
        assert p.call(caps) == -1 and "capacity" in p.msg(), caps
        assert p.report() == want_info, caps  # the needed sizes
        assert all(o.untouched() for o in p.outs()), caps
    p = Parse(env, t, fc.FINAL, nb, nn - 1, nr, names=False)  # without names their capacity does not matter
    assert p.call() == 0 and p.report() == want_info and p.bases.data().tobytes() == fc.arrays(recs)[0]


@pytest.mark.parametrize("text", [b"@x\nA\n+\nA", b"@x\nA\n+\nA\n" * 9 + b"@x\nA\n+\nA", b"@x\nA\n+\nA\n" * 700, b"@" + b"n" * 50 + b"\nA\n+\nA\n", b"\n" * 100, b"@x\n" * 50],
                         ids=["one", "ten", "700", "name", "newlines", "headers"])
def test_the_stated_upper_bounds_suffice(env, text):
    n = len(text)
    recs, want_info, _ = fc.expect(text)
    p = Parse(env, Text(text, True), fc.FINAL, n // 2, n, n // 8 + 1)
    assert p.call() == 0, p.msg()
    assert p.report() == want_info and all(o.guards_intact() for o in p.outs())
    w = fc.arrays(recs)
    assert p.bases.data()[:len(w[0])].tobytes() == w[0] and p.names.data()[:len(w[3])].tobytes() == w[3]
    assert np.array_equal(p.off.data()[:len(recs) + 1], w[2]) and np.array_equal(p.noff.data()[:len(recs) + 1], w[4])
    assert (p.bases.data()[len(w[0]):] == ah.FILL).all() and (p.names.data()[len(w[3]):] == ah.FILL).all()  # nothing behind the totals
    assert (p.off.data()[len(recs) + 1:].view(np.uint8) == ah.FILL).all()


DENSE = [b"@x\nA\n+\nA\n" * 700, b"\n" * 5000, b"@x\nA\n+\nA\n" * 300 + b"\n" * 3000]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("text", DENSE, ids=["700", "newlines", "records_then_newlines"])
def test_a_text_denser_than_the_workspace_estimate_on_a_new_context(env, text, device):
    """The workspace of a context only grows, so the repeat of the launches after an overflow of the newline positions runs only
    where a dense text is the first call of a context: more newlines than the n / 16 + 64 positions the entry point provides."""
    assert text.count(b"\n") > len(text) // 16 + 64 + 4
    fresh = dict(env, h=ah.new_context(env["_lib"], env["lib"], env["m"], GO, GE, None))
    try:
        for flags in (fc.FINAL, 0):  # the first call overflows and repeats; the second finds the larger workspace
            check(fresh, text, flags, device, what="dense first")
        check(fresh, fc.mixed_file(40, 1, 400, seed=11), fc.FINAL | fc.NAME_TO_BLANK, device, what="normal after dense")
        check(fresh, text[:len(text) // 2], fc.FINAL, device, shift=3 if device else 0, what="dense again")
    finally:
        env["lib"].zsw_destroy(fresh["h"])


# ---- NULL outputs, determinism, argument errors ------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_null_outputs(env, device):
    text = fc.mixed_file(20, 1, 70, seed=2)
    recs, want_info, _ = fc.expect(text)
    w = fc.arrays(recs)
    for quals, names in ((False, True), (True, False), (False, False)):
        p = Parse(env, Text(text, device), fc.FINAL, len(w[0]), len(w[3]), len(recs), quals=quals, names=names)
        assert p.call() == 0, p.msg()
        assert p.report() == want_info and all(o.guards_intact() for o in p.outs())
        assert p.bases.data().tobytes() == w[0] and np.array_equal(p.off.data(), w[2])
        assert not quals or p.quals.data().tobytes() == w[1]
        assert not names or (p.names.data().tobytes() == w[3] and np.array_equal(p.noff.data(), w[4]))


def test_two_calls_give_identical_arrays(env):
    parts = [fc.rec(b"r%d" % i, fc.seq_of(1 + i % 200, i), fc.qual_of(1 + i % 200, i)) for i in range(2000)]
    for i in range(1500, 2000, 7):  # many failing records: the lowest one is the same every time
        parts[i] = fc.FAULTS[1 + i % 8]
    text = b"".join(parts)
    n = len(text)
    runs = []
    for _ in range(2):
        p = Parse(env, Text(text, True), fc.FINAL, n // 2, n, n // 8 + 1)
        assert p.call() == 0
        runs.append((p.report(), [o.fetch().tobytes() for o in p.outs()]))
    assert runs[0] == runs[1] and runs[0][0][4:6] == [1 + 1500 % 8, 1500]


def test_argument_errors_write_nothing(env):
    _lib, lib, h = env["_lib"], env["lib"], env["h"]
    text = fc.mixed_file(6, 5, 30, seed=4)
    t = Text(text, True)
    n = len(text)

    def fresh():
        return Parse(env, t, fc.FINAL, n // 2, n, n // 8 + 1)

    def call(p, **kw):
        a = dict(h=h, text=t.ptr, n=n, mem=_lib.MEM_DEVICE, flags=fc.FINAL, bases=p.bases.ptr, quals=p.quals.ptr, base_cap=n // 2, off=p.off.ptr, names=p.names.ptr,
                 name_cap=n, noff=p.noff.ptr, record_cap=n // 8 + 1, info=p.info)
        a.update(kw)
        return lib.zsw_fastq_parse_batch(a["h"], a["text"], a["n"], a["mem"], a["flags"], a["bases"], a["quals"], a["base_cap"], a["off"], a["names"], a["name_cap"],
                                         a["noff"], a["record_cap"], a["info"], None)

    p = fresh()
    bad = [dict(h=None), dict(info=None), dict(text=None), dict(flags=4), dict(flags=fc.FINAL | 8), dict(mem=7), dict(bases=None), dict(off=None), dict(names=None),
           dict(noff=None), dict(quals=p.bases.ptr), dict(names=p.bases.ptr + 1), dict(bases=t.ptr + 3), dict(off=t.ptr), dict(noff=p.off.ptr + 8),
           dict(names=t.ptr + n - 1)]
    for kw in bad:
        assert call(p, **kw) == -1, kw
        assert all(o.untouched() for o in p.outs()) and p.report() == [0xA5A5A5A5] * 9, kw
    assert call(p, text=None, n=0) == 0 and p.report() == [0] * 9  # no text is needed for no bytes
    assert call(fresh()) == 0


# ---- end to end on one stream ------------------------------------------------------------------------------------------------

def test_parse_align_annotate_sam_on_one_stream(env):
    import torch

    from zoe_amd import records

    _lib, lib, h = env["_lib"], env["lib"], env["h"]
    rs = ah.mixed_set("fastq-mixed", env["ref"], 300, 0, 77)
    reads = [r for r in rs.reads if r]
    rng = np.random.default_rng(8)
    quals = [bytes(rng.integers(33, 127, len(r), dtype=np.uint8)) for r in reads]
    text = b"".join(fc.rec(b"read%d extra words\tmore" % i, r, q, eol=b"\r\n" if i % 5 == 0 else b"\n") for i, (r, q) in enumerate(zip(reads, quals)))
    host_records = list(records.FastQReader(__import__("io").BytesIO(text)))
    want = records.align_fastq_to_sam_text(host_records, env["ref"], "synthref", env["m"], GO, GE, nm=True, three_pass=True)

    stream = torch.cuda.Stream()
    n_bytes = len(text)
    t = Text(text, True)
    p = Parse(env, t, fc.FINAL | fc.NAME_TO_BLANK, n_bytes // 2, n_bytes, n_bytes // 8 + 1, stream=stream)
    assert p.call() == 0, p.msg()
    n = p.report()[0]
    assert n == len(reads) and p.report()[4] == 0
    b = _lib.ZswBatch()
    b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem, b.encoding = p.bases.ptr, p.off.ptr, 0, n, _lib.MEM_DEVICE, 0
    o = {k: ah.Out(n, ah.DTYPES[k], True) for k in ("aln", "status", "tier")}
    cap = 32 * n + 64
    inc, op = ah.Out(cap, np.uint32, True), ah.Out(cap, np.uint8, True)
    total = C.c_uint64(0)
    sp = ah.stream_ptr(stream)
    assert lib.zsw_align_3pass_batch_from(h, C.byref(b), 8, 256, 0, o["aln"].ptr, o["status"].ptr, o["tier"].ptr, inc.ptr, op.ptr, cap, C.byref(total), sp) == 0
    stats = ah.Out(n, STATS_DTYPE, True)
    out_total = C.c_uint64(0)
    assert lib.zsw_annotate_batch(h, C.byref(b), 0, o["aln"].ptr, o["status"].ptr, inc.ptr, op.ptr, int(total.value), stats.ptr, None, None, None, 0,
                                  C.byref(out_total), sp) == 0, lib.zsw_last_error_string(h).decode()
    f = _lib.ZswSamFields()
    f.qnames, f.qname_offsets, f.quals, f.stats = p.names.ptr, p.noff.ptr, p.quals.ptr, stats.ptr
    f.rname, f.rname_len, f.mapq = b"synthref", 8, 255
    sam = ah.Out(len(want), np.uint8, True)
    n_out, n_bad = C.c_uint64(0), C.c_uint64(0)
    assert lib.zsw_sam_batch(h, C.byref(b), C.byref(f), 0, o["aln"].ptr, o["status"].ptr, inc.ptr, op.ptr, int(total.value), sam.ptr, len(want), C.byref(n_out),
                             None, C.byref(n_bad), sp) == 0, lib.zsw_last_error_string(h).decode()
    stream.synchronize()
    assert int(n_out.value) == len(want) and int(n_bad.value) == 0
    assert sam.data().tobytes() == want and sam.guards_intact()


# ---- the Python layer --------------------------------------------------------------------------------------------------------

def test_python_layer_records_and_errors(env):
    import io

    from zoe_amd import records

    by_name = dict(fc.CASES)
    for name in ("valid_lf", "valid_crlf", "valid_no_final_newline", "name_utf8", "name_blanks", "seq_lengths", "name_lengths", "plus_name"):
        text = by_name[name]
        fq = records.fastq_batch_from_text(text)
        assert fq.records() == list(records.FastQReader(io.BytesIO(text))), name
        assert fq.consumed == len(text) and len(fq) == len(fq.records())
    assert records.fastq_batch_from_text(b"").records() == []
    part = records.fastq_batch_from_text(by_name["stops_after_line2_unterminated"], final=False)
    assert len(part) == 5 and part.consumed == len(fc.five({}))
    blank = records.fastq_batch_from_text(by_name["name_blanks"], name_to_blank=True).records()
    assert [r.header for r in blank] == ["r1", "r2", "", "", "tail", ""]
    for code in range(1, 9):  # the reader's own message, one case per code
        text = by_name[f"code{code}_at2"]
        with pytest.raises(records.FastQError) as host:
            list(records.FastQReader(io.BytesIO(text)))
        with pytest.raises(records.FastQError) as dev:
            records.fastq_batch_from_text(text)
        assert str(dev.value) == str(host.value) and fc.code_of(str(dev.value)) == code


def test_python_twin_from_text_equals_the_twin_from_records(env):
    import io

    from zoe_amd import records, synth

    reads = synth.reads_host(env["ref"], 5, 64, 150)  # cut to 60 .. 123 bases below
    text = b"".join(fc.rec(b"q%d some words" % i, r.tobytes()[:60 + i], fc.qual_of(60 + i, i)) for i, r in enumerate(reads))
    host = list(records.FastQReader(io.BytesIO(text)))
    for kw in (dict(), dict(nm=True, verbose_cigar=True, three_pass=True)):
        want = records.align_fastq_to_sam_text(host, env["ref"], "synthref", env["m"], GO, GE, **kw)
        assert records.align_fastq_text_to_sam_text(text, env["ref"], "synthref", env["m"], GO, GE, **kw) == want
    assert records.align_fastq_text_to_sam_text(b"", env["ref"], "synthref", env["m"], GO, GE) == b""


def test_python_twin_from_text_cuts_the_name_at_the_first_space_or_tab(env):
    """The one documented difference between the twins: QNAME from text ends in front of the first space or tab of the header
    (the driver's rule), QNAME from records is `header.split()[0]`. Every other column is the same."""
    import io

    from zoe_amd import records, synth

    headers = [b" lead word", b"\tlead", b"a\x0bb c", b"a\x0cb\td", b"plain x", b"caf\xc3\xa9\xc2\xa0x y"]
    from_text = [b"", b"", b"a\x0bb", b"a\x0cb", b"plain", b"caf\xc3\xa9\xc2\xa0x"]
    from_records = [b"lead", b"lead", b"a", b"a", b"plain", b"caf\xc3\xa9"]  # str.split also splits at U+000B, U+000C and U+00A0
    reads = synth.reads_host(env["ref"], 6, len(headers), 150)
    text = b"".join(fc.rec(h, r.tobytes()[:70 + i], fc.qual_of(70 + i, i)) for i, (h, r) in enumerate(zip(headers, reads)))
    host = list(records.FastQReader(io.BytesIO(text)))
    a = records.align_fastq_text_to_sam_text(text, env["ref"], "synthref", env["m"], GO, GE, nm=True).split(b"\n")
    b = records.align_fastq_to_sam_text(host, env["ref"], "synthref", env["m"], GO, GE, nm=True).split(b"\n")
    assert len(a) == len(b) == len(headers) + 1 and a[-1] == b[-1] == b""
    assert [ln.split(b"\t", 1)[0] for ln in a[:-1]] == from_text and [ln.split(b"\t", 1)[0] for ln in b[:-1]] == from_records
    assert [ln.split(b"\t", 1)[1] for ln in a[:-1]] == [ln.split(b"\t", 1)[1] for ln in b[:-1]]
