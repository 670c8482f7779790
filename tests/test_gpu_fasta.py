"""GPU tests of zsw_fasta_parse_batch through ctypes and the C ABI: every output array and all nine report words against what
records.FastaReader yields over the same bytes (tests/fasta_cases.py; clean in the host model first, tests/test_fasta_model.py).

Every call gets output arrays of exactly the sizes the expectation has, between canary entries: a byte written past a capacity, or
not written inside it, shows. Shapes are the smallest at which the kernels can go wrong: the case list in device and host memory
under every flag set, continued texts too; texts of 0, 1, 15, 16, 17 bytes and one byte either side of a tile; a '>', a "\\r\\n",
the end of a header and the first base of a body on either side of a tile edge; the text at device addresses base + 1, 3, 15; 3,000
records of 1-5 bases (several per granule, hundreds per tile); one record of five tiles wrapped with CRLF and one on a single line;
one block of records +- 1; a buffer cut at every byte of its last two records without FINAL, and the restart with CONTINUED; the
capacity protocol; NULL names; a text with more '>' than the workspace estimate as the first call of a new context; two runs; the
argument errors; a parsed record as the reference without a copy; FASTA reads -> 3-pass alignment -> SAM on one stream; the Python
layer."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import abi_helpers as ah
import fasta_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"FQ_TILE = (\d+);", open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_text.hpp")).read()).group(1))
BLOCK_RECORDS = int(re.search(r"FA_BLOCK_RECORDS = (\d+);", open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_fasta.hpp")).read()).group(1))
GO, GE = -10, -1


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib, synth

    lib = _lib.load()
    assert hasattr(lib, "zsw_fasta_parse_batch")
    m = zoe_amd.WeightMatrix.new(zoe_amd.DNA_PROFILE_MAP, 2, -5, b"N")
    ref = synth.reference_host(2000)
    h = ah.new_context(_lib, lib, m, GO, GE, ref)
    yield {"za": zoe_amd, "_lib": _lib, "lib": lib, "m": m, "ref": ref, "h": h}
    lib.zsw_destroy(h)


def test_the_constants_the_shapes_are_built_from():
    assert TILE == 4096 and BLOCK_RECORDS == 8


class Text:
    """the bytes of a call, in device memory at base + shift or in host memory"""

    def __init__(self, text: bytes, device: bool, shift: int = 0):
        self.n, self.device = len(text), device
        a = np.full(shift + len(text) + 1, 0x3E, dtype=np.uint8)  # '>' in front of and behind the text: a load outside it is counted
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
    """one zsw_fasta_parse_batch call with output arrays of the given capacities between canary entries"""

    def __init__(self, env, text: Text, flags, base_cap, name_cap, record_cap, names=True, stream=None):
        self.env, self.text, self.flags, self.stream = env, text, flags, stream
        dev = text.device
        self.caps = (base_cap, name_cap, record_cap)
        self.bases = ah.Out(base_cap, np.uint8, dev)
        self.off = ah.Out(record_cap + 1, np.uint64, dev)
        self.names = ah.Out(name_cap, np.uint8, dev) if names else None
        self.noff = ah.Out(record_cap + 1, np.uint64, dev) if names else None
        self.info = (C.c_uint64 * 9)(*([0xA5A5A5A5] * 9))

    def outs(self):
        return [o for o in (self.bases, self.off, self.names, self.noff) if o is not None]

    def call(self, caps=None):
        env, t = self.env, self.text
        base_cap, name_cap, record_cap = self.caps if caps is None else caps
        ptr = lambda o: None if o is None else o.ptr
        return env["lib"].zsw_fasta_parse_batch(env["h"], t.ptr, t.n, env["_lib"].MEM_DEVICE if t.device else env["_lib"].MEM_HOST, self.flags, self.bases.ptr, base_cap,
                                                self.off.ptr, ptr(self.names), name_cap, ptr(self.noff), record_cap, self.info, ah.stream_ptr(self.stream))

    def msg(self):
        return self.env["lib"].zsw_last_error_string(self.env["h"]).decode()

    def report(self):
        return [int(x) for x in self.info]


def check(env, text: bytes, flags=fc.FINAL, device=True, shift=0, what=""):
    """the call with exactly the capacities the expectation needs -> (records, report)"""
    recs, want_info, _ = fc.expect(text, flags)
    w_bases, w_off, w_names, w_noff = fc.arrays(recs)
    p = Parse(env, Text(text, device, shift), flags, len(w_bases), len(w_names), len(recs))
    rc = p.call()
    tag = (what, flags, device, shift)
    assert rc == 0, (tag, rc, p.msg())
    assert p.report() == want_info, (tag, dict(zip(fc.INFO, p.report())), dict(zip(fc.INFO, want_info)))
    assert all(o.guards_intact() for o in p.outs()), tag
    assert p.bases.data().tobytes() == w_bases and p.names.data().tobytes() == w_names, tag
    assert np.array_equal(p.off.data(), w_off) and np.array_equal(p.noff.data(), w_noff), tag
    return recs, want_info


# ---- the case list -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("flags", fc.FLAG_SETS)
def test_the_case_list(env, device, flags):
    for name, text in fc.CASES:
        check(env, text, flags, device, what=name)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_continued_texts(env, device):
    cont = fc.continued_cases()
    for flags in (fc.FINAL | fc.CONTINUED, fc.CONTINUED | fc.NAME_TO_BLANK):
        for name, text in cont[::2] if flags & fc.FINAL else cont[1::2]:
            check(env, text, flags, device, what=name)


# ---- word and tile edges -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    text = fc.mixed_file(40, 1, 700, seed=3)
    assert len(text) > 2 * TILE + 17
    return text


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1])
def test_text_lengths_at_the_word_and_tile_edges(env, big, n):
    for flags in (fc.FINAL, 0):
        for device in (True, False):
            check(env, big[:n], flags, device, what=f"cut{n}")


def edge_texts():
    """(what, text, shift): a '>', the last byte of a header, the '\\n' of a "\\r\\n" and the first base of a body, each as the last byte
    of a tile and as the first byte of the next, at the first tile edge and the third"""
    tail = b">hdr name\r\nACGT\r\nAC\r\n>z\r\nA\r\n"
    out = []
    for what, idx in (("gt", 0), ("header_end", 8), ("crlf", 10), ("first_base", 11)):
        for edge in (TILE, 3 * TILE):
            for v in (edge - 1, edge):
                for shift in (0, 5):
                    text = b">p\r\n" + fc.seq_of(v - shift - 6 - idx) + b"\r\n" + tail
                    assert text[v - shift] == tail[idx]
                    out.append((f"{what}_at{v}_shift{shift}", text, shift))
    return out


def test_either_side_of_a_tile_edge(env):
    for what, text, shift in edge_texts():
        for flags in (fc.FINAL, fc.FINAL | fc.CONTINUED, fc.NAME_TO_BLANK):
            recs, info = check(env, text, flags, True, shift, what=what)
            assert info[4] == 0 and info[0] == (3 if flags & fc.FINAL else 2)


@pytest.mark.parametrize("shift", [1, 3, 15])
def test_the_text_at_unaligned_device_addresses(env, big, shift):
    for n in (17, TILE - shift, TILE - shift + 1, len(big)):
        check(env, big[:n], fc.FINAL, True, shift, what=f"shift{shift} cut{n}")
    check(env, dict(fc.CASES)["code6_at2"], fc.FINAL, True, shift)
    check(env, dict(fc.CASES)["blank_lines_in_bodies"], 0, True, shift)


# ---- record counts and shapes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, BLOCK_RECORDS - 1, BLOCK_RECORDS, BLOCK_RECORDS + 1])
def test_record_counts(env, n):
    recs, info = check(env, fc.mixed_file(n, 1, 400, seed=n), fc.FINAL | fc.NAME_TO_BLANK, True, what=f"n{n}")
    assert info[0] == n and info[4] == 0 and (n == 1 or info[7:9] == [1, 400])


def test_many_tiny_records(env):
    """3,000 records of 1-5 bases with one-byte names: several records start inside one 16-byte granule, hundreds inside one tile"""
    text = b"".join(b">" + b"abcdefghij"[i % 10:i % 10 + 1] + b"\n" + fc.seq_of(1 + i % 5, i) + (b"\r\n" if i % 3 == 0 else b"\n") for i in range(3000))
    gts = [i for i, c in enumerate(text) if c == 62]
    assert min(b - a for a, b in zip(gts, gts[1:])) <= 5 and len(text) // TILE >= 4 and len(gts) * TILE // len(text) > 300
    for flags in (fc.FINAL, 0):
        recs, info = check(env, text, flags, True, what="tiny")
        assert info[0] == (3000 if flags else 2999) and info[4] == 0 and info[7:9] == [1, 5]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_one_long_record(env, device):
    """one record of five tiles wrapped at 60 columns with CRLF, and one of five tiles on a single line, each between two short ones"""
    seq = fc.seq_of(5 * TILE + 7, 3)
    for body in (fc.wrap(seq, 60, b"\r\n"), seq + b"\n", seq):
        text = b">first\nACGT\n>long one\r\n" + body + (b">last\nAC\n" if body.endswith(b"\n") else b"")
        recs, info = check(env, text, fc.FINAL, device, shift=3 if device else 0, what="long")
        assert info[4] == 0 and info[8] == len(seq) and recs[1] == (b"long one", seq)


def test_the_lowest_failing_record_of_many(env):
    parts = [fc.rec(b"r%d x" % i, fc.seq_of(1 + i % 90, i), width=30) for i in range(3000)]
    for i in (2999, 2500, 1777, 1778):
        parts[i] = fc.FAULTS_LATER[3 + i % 3]  # MISSING_HEADER, GT_IN_HEADER, MISSING_SEQUENCE
    recs, info = check(env, b"".join(parts), fc.FINAL, True)
    assert info[4:6] == [3 + 1777 % 3, 1777] and len(recs) == 1777


# ---- without FINAL -----------------------------------------------------------------------------------------------------------

def test_without_final_a_buffer_cut_at_every_byte_of_its_last_two_records_and_the_restart(env):
    text = fc.mixed_file(5, 3, 90, seed=5, width=20) + fc.rec(b"crlf one", b"ACGTACGTAC", eol=b"\r\n", width=4) + fc.rec(b"last", b"ACG")
    gts = [i for i, c in enumerate(text) if c == 62]
    all_recs = fc.expect(text)[0]
    assert len(all_recs) == 7
    for n in range(gts[-2], len(text) + 1):
        recs, info = check(env, text[:n], 0, True, what=f"cut{n}")
        full = sum(1 for i in gts if i < n) - 1
        assert info[0] == full and info[3] == gts[full] and info[4] == 0
        # the restart at CONSUMED once the rest of the file is there: together the records of the one call
        rest, rest_info = check(env, text[info[3]:], fc.FINAL | fc.CONTINUED, True, what=f"restart{n}")
        assert recs + rest == all_recs and rest_info[4] == 0


# ---- the capacity protocol ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_capacity_protocol(env, device):
    text = fc.mixed_file(40, 1, 90, seed=9, width=25)
    recs, want_info, _ = fc.expect(text)
    nb, nn, nr = want_info[1], want_info[2], want_info[0]
    t = Text(text, device)
    info = (C.c_uint64 * 9)()
    mem = env["_lib"].MEM_DEVICE if device else env["_lib"].MEM_HOST
    assert env["lib"].zsw_fasta_parse_batch(env["h"], t.ptr, t.n, mem, fc.FINAL, None, 0, None, None, 0, None, 0, info, None) == 0  # the sizing call
    assert [int(x) for x in info] == want_info
    for caps in ((nb - 1, nn, nr), (nb, nn - 1, nr), (nb, nn, nr - 1), (0, 0, 0)):
        p = Parse(env, t, fc.FINAL, nb, nn, nr)
        assert p.call(caps) == -1 and "capacity" in p.msg(), caps
        assert p.report() == want_info, caps  # the needed sizes
        assert all(o.untouched() for o in p.outs()), caps
    p = Parse(env, t, fc.FINAL, nb, nn - 1, nr, names=False)  # without names their capacity does not matter
    assert p.call() == 0 and p.report() == want_info and p.bases.data().tobytes() == fc.arrays(recs)[0]
    assert np.array_equal(p.off.data(), fc.arrays(recs)[1]) and all(o.guards_intact() for o in p.outs())


@pytest.mark.parametrize("text", [b">a\nA", b">a\nA\n" * 9 + b">a\nA", b">a\nA\n" * 700, b">" + b"n" * 50 + b"\nA\n", b">a\n" + b"A" * 300, b">" * 100, b">a\n" * 50],
                         ids=["one", "ten", "700", "name", "bases", "gts", "headers"])
def test_the_stated_upper_bounds_suffice(env, text):
    n = len(text)
    recs, want_info, _ = fc.expect(text)
    p = Parse(env, Text(text, True), fc.FINAL, n, n, n // 4 + 1)
    assert p.call() == 0, p.msg()
    assert p.report() == want_info and all(o.guards_intact() for o in p.outs())
    w = fc.arrays(recs)
    assert p.bases.data()[:len(w[0])].tobytes() == w[0] and p.names.data()[:len(w[2])].tobytes() == w[2]
    assert np.array_equal(p.off.data()[:len(recs) + 1], w[1]) and np.array_equal(p.noff.data()[:len(recs) + 1], w[3])
    assert (p.bases.data()[len(w[0]):] == ah.FILL).all() and (p.names.data()[len(w[2]):] == ah.FILL).all()  # nothing behind the totals
    assert (p.off.data()[len(recs) + 1:].view(np.uint8) == ah.FILL).all() and (p.noff.data()[len(recs) + 1:].view(np.uint8) == ah.FILL).all()


DENSE = [b">a\nA\n" * 700, b">" * 5000, b">a\nA\n" * 300 + b">" * 3000]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("text", DENSE, ids=["700", "gts", "records_then_gts"])
def test_a_text_denser_than_the_workspace_estimate_on_a_new_context(env, text, device):
    """The workspace of a context only grows, so the repeat of the launches after an overflow of the '>' positions runs only where a
    dense text is the first call of a context: more '>' than the n / 64 + 64 positions the entry point provides."""
    assert text.count(b">") > len(text) // 64 + 64 + 4
    fresh = dict(env, h=ah.new_context(env["_lib"], env["lib"], env["m"], GO, GE, None))
    try:
        for flags in (fc.FINAL, 0):  # the first call overflows and repeats; the second finds the larger workspace
            check(fresh, text, flags, device, what="dense first")
        check(fresh, fc.mixed_file(40, 1, 400, seed=11), fc.FINAL | fc.NAME_TO_BLANK, device, what="normal after dense")
        check(fresh, text[:len(text) // 2], fc.FINAL, device, shift=3 if device else 0, what="dense again")
    finally:
        env["lib"].zsw_destroy(fresh["h"])


# ---- NULL names, determinism, argument errors --------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_null_names(env, device):
    text = fc.mixed_file(20, 1, 70, seed=2, width=17)
    recs, want_info, _ = fc.expect(text)
    w = fc.arrays(recs)
    p = Parse(env, Text(text, device), fc.FINAL, len(w[0]), 0, len(recs), names=False)
    assert p.call() == 0, p.msg()
    assert p.report() == want_info and all(o.guards_intact() for o in p.outs())
    assert p.bases.data().tobytes() == w[0] and np.array_equal(p.off.data(), w[1])


def test_two_calls_give_identical_arrays(env):
    parts = [fc.rec(b"r%d" % i, fc.seq_of(1 + i % 200, i), width=50) for i in range(2000)]
    for i in range(1500, 2000, 7):  # many failing records: the lowest one is the same every time
        parts[i] = fc.FAULTS_LATER[3 + i % 3]
    text = b"".join(parts)
    n = len(text)
    runs = []
    for _ in range(2):
        p = Parse(env, Text(text, True), fc.FINAL, n, n, n // 4 + 1)
        assert p.call() == 0
        runs.append((p.report(), [o.fetch().tobytes() for o in p.outs()]))
    assert runs[0] == runs[1] and runs[0][0][4:6] == [3 + 1500 % 3, 1500]


def test_argument_errors_write_nothing(env):
    _lib, lib, h = env["_lib"], env["lib"], env["h"]
    text = fc.mixed_file(6, 5, 30, seed=4)
    t = Text(text, True)
    n = len(text)

    def fresh():
        return Parse(env, t, fc.FINAL, n, n, n // 4 + 1)

    def call(p, **kw):
        a = dict(h=h, text=t.ptr, n=n, mem=_lib.MEM_DEVICE, flags=fc.FINAL, bases=p.bases.ptr, base_cap=n, off=p.off.ptr, names=p.names.ptr, name_cap=n, noff=p.noff.ptr,
                 record_cap=n // 4 + 1, info=p.info)
        a.update(kw)
        return lib.zsw_fasta_parse_batch(a["h"], a["text"], a["n"], a["mem"], a["flags"], a["bases"], a["base_cap"], a["off"], a["names"], a["name_cap"], a["noff"],
                                         a["record_cap"], a["info"], None)

    p = fresh()
    host_text = np.frombuffer(b"x" + text, dtype=np.uint8).copy()
    bad = [dict(h=None), dict(info=None), dict(text=None), dict(flags=8), dict(flags=fc.FINAL | 16), dict(mem=7), dict(bases=None), dict(off=None), dict(names=None),
           dict(noff=None), dict(names=p.bases.ptr + 1), dict(bases=t.ptr + 3), dict(off=t.ptr), dict(noff=p.off.ptr + 8), dict(names=t.ptr + n - 1),
           dict(flags=fc.FINAL | fc.CONTINUED, text=t.ptr + 1, n=n - 1),                                # a continued text in device memory that starts with 'r'
           dict(flags=fc.CONTINUED, text=host_text.ctypes.data, n=n + 1, mem=_lib.MEM_HOST),             # ... in host memory
           dict(flags=fc.CONTINUED, text=None, n=0)]                                                     # ... that is empty
    for kw in bad:
        assert call(p, **kw) == -1, kw
        assert all(o.untouched() for o in p.outs()) and p.report() == [0xA5A5A5A5] * 9, kw
    assert call(p, text=None, n=0, flags=0) == 0 and p.report() == [0] * 9  # no text is needed for no bytes
    assert call(p, text=None, n=0) == 0 and p.report() == [0, 0, 0, 0, fc.NO_DATA, 0, 0, 0, 0]
    assert call(fresh()) == 0


# ---- a parsed record as the reference, FASTA reads to SAM --------------------------------------------------------------------

def test_a_parsed_record_is_the_reference_without_a_copy(env):
    """parse a three-record file, zsw_set_reference(ZSW_MEM_DEVICE) on record 1 where the parser left it, score a batch: the scores
    of the same call with that sequence set from host memory"""
    _lib, lib = env["_lib"], env["lib"]
    from zoe_amd import synth

    ref1 = bytes(env["ref"][:1500])
    text = fc.rec(b"zero", fc.seq_of(333, 1), width=70) + fc.rec(b"one the reference", ref1, eol=b"\r\n", width=60) + fc.rec(b"two", fc.seq_of(100, 2), width=70)
    reads = [r.tobytes()[:80 + i] for i, r in enumerate(synth.reads_host(ref1, 11, 40, 150))]
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    offsets = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    b = _lib.ZswBatch()
    b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem, b.encoding = bases.ctypes.data, offsets.ctypes.data, 0, len(reads), _lib.MEM_HOST, 0
    fresh = dict(env, h=ah.new_context(_lib, lib, env["m"], GO, GE, None))
    try:
        h = fresh["h"]
        n = len(text)
        p = Parse(fresh, Text(text, True, shift=1), fc.FINAL | fc.NAME_TO_BLANK, n, n, n // 4 + 1)
        assert p.call() == 0 and p.report()[:2] == [3, 333 + 1500 + 100] and p.report()[4] == 0
        off = p.off.data()
        assert p.names.data()[:int(p.report()[2])].tobytes() == b"zeroonetwo"
        results = []
        for ptr, mem in ((p.bases.ptr + int(off[1]), _lib.MEM_DEVICE), (np.frombuffer(ref1, dtype=np.uint8).ctypes.data, _lib.MEM_HOST)):
            assert lib.zsw_set_reference(h, ptr, int(off[2] - off[1]), mem) == 0
            score, status = np.zeros(len(reads), np.uint32), np.full(len(reads), 0xA5, np.uint8)
            assert lib.zsw_score_batch_from(h, C.byref(b), 8, 256, score.ctypes.data, status.ctypes.data, None, None) == 0, lib.zsw_last_error_string(h).decode()
            results.append((score.tobytes(), status.tobytes()))
            assert (score > 0).any()
        assert results[0] == results[1]
    finally:
        lib.zsw_destroy(fresh["h"])


def test_fasta_reads_align_sam_on_one_stream(env):
    """FASTA reads -> zsw_align_3pass_batch_from -> zsw_sam_batch with quals == NULL, on one stream: the text of the host path over
    the same records, QUAL '*'"""
    import torch

    from zoe_amd import records

    _lib, lib, h = env["_lib"], env["lib"], env["h"]
    rs = ah.mixed_set("fasta-mixed", env["ref"], 200, 0, 78)
    reads = [r for r in rs.reads if r]
    text = b"".join(fc.rec(b"read%d extra words\tmore" % i, r, eol=b"\r\n" if i % 5 == 0 else b"\n", width=60 if i % 2 else None) for i, r in enumerate(reads))
    host = list(records.FastaReader(io.BytesIO(text)))
    assert [r.sequence for r in host] == reads
    fq = [records.FastQ(r.name.decode(), r.sequence, b"") for r in host]
    want = "".join(str(r) + "\n" for r in records.align_fastq_to_sam(fq, env["ref"], "synthref", env["m"], GO, GE, three_pass=True)).encode()
    assert want.count(b"\t*\tAS:i:") > 100

    stream = torch.cuda.Stream()
    n_bytes = len(text)
    p = Parse(env, Text(text, True), fc.FINAL | fc.NAME_TO_BLANK, n_bytes, n_bytes, n_bytes // 4 + 1, stream=stream)
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
    f = _lib.ZswSamFields()
    f.qnames, f.qname_offsets, f.quals, f.stats = p.names.ptr, p.noff.ptr, None, None
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
    from zoe_amd import records

    by_name = dict(fc.CASES)
    for name in ("valid_lf", "valid_crlf", "valid_no_final_newline", "wrapped", "wrapped_crlf", "name_high_bytes", "name_blanks", "blank_lines_in_bodies", "sequence_bytes",
                 "lone_cr_in_first_header"):
        text = by_name[name]
        fa = records.fasta_batch_from_text(text)
        assert fa.records() == list(records.FastaReader(io.BytesIO(text))), name
        assert fa.consumed == len(text) and len(fa) == len(fa.records())
    part = records.fasta_batch_from_text(by_name["header_without_line_break_at_the_end"], final=False)
    assert len(part) == 1 and part.consumed == 8
    rest = records.fasta_batch_from_text(by_name["valid_lf"][part.consumed:], continued=True)
    assert [r.name for r in rest.records()] == [b"bb", b"ccc"]
    blank = records.fasta_batch_from_text(by_name["name_blanks"], name_to_blank=True).records()
    assert [r.name for r in blank] == [b"r1", b"r2", b"", b"", b"tail", b"", b""]
    for name, code in [(f"code{c}_at2", c) for c in (3, 4, 5, 6)] + [("empty", fc.NO_DATA), ("text_first", fc.MISSING_GT), ("cr_gt_quirk", fc.GT_IN_HEADER)]:
        text = by_name[name]
        with pytest.raises(records.FastaError) as host:
            list(records.FastaReader(io.BytesIO(text)))
        with pytest.raises(records.FastaError) as dev:
            records.fasta_batch_from_text(text)
        assert str(dev.value).endswith(str(host.value)) and dev.value.code == host.value.code == code and dev.value.offset == host.value.offset, name


def test_python_layer_reference_and_reads(env):
    """`.sequence(r)` is a device view `set_reference` takes; `.as_read_batch()` feeds the profile classes: the alignments of the
    same reads built from host records"""
    from zoe_amd import records, synth
    from zoe_amd.alignment import SeqSrc, SwContext, into_local_profile

    ref1 = bytes(env["ref"][:900])
    fa = records.fasta_batch_from_text(fc.rec(b"a", b"ACGT") + fc.rec(b"ref", ref1, width=60) + fc.rec(b"c", b"GG"))
    view = fa.sequence(1)
    assert view.is_cuda and view.cpu().numpy().tobytes() == ref1 and view.data_ptr() == fa.bases.data_ptr() + 4
    with pytest.raises(IndexError):
        fa.sequence(3)
    SwContext.get(0).set_reference(view)
    reads = [r.tobytes()[:90 + i] for i, r in enumerate(synth.reads_host(ref1, 5, 8, 150))]
    text = b"".join(fc.rec(b"q%d" % i, r, width=50) for i, r in enumerate(reads))
    batch = records.fasta_batch_from_text(text, name_to_blank=True)
    got = into_local_profile(batch.as_read_batch(), env["m"], GO, GE).sw_align_from_i8(SeqSrc.Reference(ref1))
    want = into_local_profile(records.batch_from_fastq([records.FastQ("q", r, b"") for r in reads]), env["m"], GO, GE).sw_align_from_i8(SeqSrc.Reference(ref1))
    assert np.array_equal(got.status, want.status) and np.array_equal(got.records, want.records) and [got.cigar(i) for i in range(8)] == [want.cigar(i) for i in range(8)]
