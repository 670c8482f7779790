"""Helpers of the C ABI tests (test_gpu_abi_matrix.py, test_gpu_call_order.py, the pipeline test): read sets that exercise the
edges, the presentations of one read set the ABI allows (device / host, fixed / ragged / packed), output arrays with guard
entries, and one call wrapper for the score, ends, ranges and alignment entry points of both profile roles.

Plain module, no fixtures: the tests import it by name, as test_gpu_seed.py imports test_gpu_bounds."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

GUARD = 64      # extra entries in front of and behind every output array
FILL = 0xA5     # their bytes; no zsw_status has this value
S_, O_, U_, E_ = 0, 1, 2, 3
ORACLE_THREADS = 12  # the per-read oracle calls release the GIL (ctypes)

ALN_DTYPE = np.dtype(
    [("score", "<u4"), ("ref_start", "<u4"), ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"),
     ("ref_len", "<u4"), ("query_len", "<u4"), ("n_ciglets", "<u4"), ("ciglet_offset", "<u8")]
)

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- read sets ---------------------------------------------------------------------------------------------------------------

@dataclass
class ReadSet:
    name: str
    ref: bytes
    reads: list            # bytes per read
    fixed_len: int         # 0: ragged
    cls: np.ndarray        # class label per read (CLASSES)
    origin: np.ndarray     # reference position the read was cut from, -1 = none
    T: str = "i16"         # the instantiation of the direct calls on this set
    lanes: int = 16
    _flat: Optional[np.ndarray] = field(default=None, repr=False)
    _off: Optional[np.ndarray] = field(default=None, repr=False)

    @property
    def n(self) -> int:
        return len(self.reads)

    @property
    def bases(self) -> np.ndarray:
        if self._flat is None:
            cat = b"".join(self.reads)
            self._flat = np.frombuffer(cat if cat else b"\0", dtype=np.uint8).copy()
        return self._flat

    @property
    def offsets(self) -> np.ndarray:
        if self._off is None:
            self._off = np.zeros(self.n + 1, dtype=np.uint64)
            np.cumsum([len(r) for r in self.reads], out=self._off[1:])
        return self._off

    def subset(self, n: int, name: str) -> "ReadSet":
        return ReadSet(name, self.ref, self.reads[:n], self.fixed_len, self.cls[:n].copy(), self.origin[:n].copy(), self.T, self.lanes)


CLASSES = ("near", "diverged", "one_indel", "indels", "ties", "bytes", "random", "all_n", "empty")
EDGE_CLASSES = ("ties", "bytes", "all_n", "empty")
GAP_CLASSES = ("one_indel", "indels")


def _piece(rng, r: np.ndarray, length: int):
    pos = int(rng.integers(0, max(1, len(r) - length - 16)))
    return pos, r[pos:pos + length + 16].copy()


def _substitute(rng, q: np.ndarray, rate: float) -> np.ndarray:
    hit = rng.random(len(q)) < rate
    q = q.copy()
    q[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return q


def _indels(rng, q: np.ndarray, count: int, length: int, kinds=(0, 1)) -> np.ndarray:
    """`count` gap runs of 1..3 bases, away from the ends (so that the alignment keeps them); kinds: 0 insertion, 1 deletion"""
    q = q.copy()
    for k in range(count):
        p = int(rng.integers(25, max(26, min(len(q), length) - 25)))
        run = int(rng.integers(1, 4))
        if kinds[k % len(kinds)] == 0:
            q = np.insert(q, p, ACGT[rng.integers(0, 4, run)])
        else:
            q = np.delete(q, slice(p, p + run))
    return q


def _fit(rng, q: np.ndarray, length: int) -> np.ndarray:
    if len(q) < length:
        q = np.concatenate([q, ACGT[rng.integers(0, 4, length - len(q))]])
    return np.ascontiguousarray(q[:length], dtype=np.uint8)


def _one_read(rng, r: np.ndarray, length: int, cls: str, k: int):
    """one read of `length` bases of class `cls` (k: running number within the class) -> (bytes, origin)"""
    pos, q = _piece(rng, r, length)
    if cls == "near":
        q = _substitute(rng, q, 0.01)
    elif cls == "diverged":
        q = _substitute(rng, q, float(rng.uniform(0.03, 0.12)))
        if length > 80 and k % 2:
            q = _indels(rng, q, 1, length)
    elif cls == "one_indel":
        q = _indels(rng, _substitute(rng, q, 0.005), 1, length, kinds=(k % 2,)) if length > 60 else q
    elif cls == "indels":
        q = _indels(rng, _substitute(rng, q, 0.005), int(rng.integers(2, 5)), length, kinds=(k % 2, 1 - k % 2)) if length > 80 else q
    elif cls == "ties":
        pos = -1
        h = max(1, length // 3)
        kind = k % 4
        if kind == 0:    # two pieces of the reference in the opposite order: two cells hold the maximum, (early row, late column)
            a = int(rng.integers(len(r) // 2, len(r) - h - 1))   # and (late row, early column), so the two tie rules disagree
            b = int(rng.integers(0, len(r) // 2 - h - 1))
            q = np.concatenate([r[a:a + h], ACGT[rng.integers(0, 4, max(0, length - 2 * h))], r[b:b + h]])
        elif kind == 1:  # homopolymer
            q = np.full(length, ACGT[k // 4 % 4], dtype=np.uint8)
        elif kind == 2:  # dinucleotide repeat
            q = np.resize(np.array([ACGT[k // 4 % 4], ACGT[(k // 4 + 1) % 4]], dtype=np.uint8), length)
        else:            # the same piece twice
            q = np.concatenate([q[:h], q[:h], q[:h]])
    elif cls == "bytes":
        q = _substitute(rng, q, 0.01)[:length]
        kind = k % 4
        if kind == 0:
            q = np.frombuffer(q.tobytes().lower(), dtype=np.uint8).copy()
        elif kind == 1:
            q[q == ord("T")] = ord("U")
        elif kind == 2:
            q[rng.random(len(q)) < 0.1] = ord("N")
        else:
            hit = np.nonzero(rng.random(len(q)) < 0.08)[0]
            q[hit] = np.frombuffer(b"RYKMSWBDHVn-u.", dtype=np.uint8)[rng.integers(0, 14, len(hit))]
    elif cls == "random":
        pos = -1
        q = ACGT[rng.integers(0, 4, length)]
    elif cls == "all_n":
        pos = -1
        q = np.full(length, ord("N") if k % 2 == 0 else ord("n"), dtype=np.uint8)
    elif cls == "empty":
        return b"", -1
    return _fit(rng, np.asarray(q, dtype=np.uint8), length).tobytes(), pos


MIX_FIXED = (("near", 0.36), ("diverged", 0.14), ("one_indel", 0.14), ("indels", 0.12), ("ties", 0.08), ("bytes", 0.08), ("random", 0.07), ("all_n", 0.01))
MIX_RAGGED = (("near", 0.38), ("diverged", 0.10), ("one_indel", 0.14), ("indels", 0.12), ("ties", 0.06), ("bytes", 0.08), ("random", 0.07), ("all_n", 0.01), ("empty", 0.04))


def mixed_set(name: str, ref: bytes, n: int, length: int, seed: int, T: str = "i16", lanes: int = 16) -> ReadSet:
    """n reads; length > 0: all of that length, length == 0: lengths 1..400 and some empty reads. The classes are interleaved, so
    every prefix of the set (the tiny batches) and every shard holds a mix."""
    from zoe_amd import synth

    rng = np.random.default_rng(seed)
    r = np.frombuffer(ref, dtype=np.uint8)
    mix = MIX_FIXED if length else MIX_RAGGED
    labels = np.concatenate([np.full(max(1, int(round(share * n))), CLASSES.index(c)) for c, share in mix])
    labels = np.resize(labels, n)
    rng.shuffle(labels)
    synth_reads = synth.reads_host(ref, seed, n, length or 400)  # the bench generator's reads for part of the `near` class
    counts = dict.fromkeys(CLASSES, 0)
    reads, origin = [], np.full(n, -1, dtype=np.int64)
    for i in range(n):
        cls = CLASSES[labels[i]]
        k = counts[cls]
        counts[cls] += 1
        L = length or int(rng.integers(1, 401))
        if cls == "near" and k % 2:
            reads.append(synth_reads[i, :L].tobytes())
            continue
        q, origin[i] = _one_read(rng, r, L, cls, k)
        reads.append(q)
    return ReadSet(name, ref, reads, length, labels.astype(np.int64), origin, T, lanes)


def sample_of(rs: ReadSet, size: int = 300) -> np.ndarray:
    """The fixed sample the per-read oracle checks: reads of the edge classes and reads with gaps first (round robin over the
    classes, four fifths of the sample at most), the rest evenly spaced over the other reads."""
    by_cls = [list(np.nonzero(rs.cls == CLASSES.index(c))[0]) for c in EDGE_CLASSES + GAP_CLASSES + ("diverged",)]
    picked, want = [], min(size * 4 // 5, sum(len(b) for b in by_cls))
    while len(picked) < want:
        for b in by_cls:
            if b and len(picked) < want:
                picked.append(int(b.pop(0)))
    rest = np.setdiff1d(np.arange(rs.n), np.array(picked, dtype=np.int64))
    fill = min(len(rest), max(0, size - len(picked)))
    if fill:
        picked += [int(x) for x in rest[np.linspace(0, len(rest) - 1, fill).astype(np.int64)]]
    return np.array(sorted(set(picked)), dtype=np.int64)


def pmap(fn, items):
    with ThreadPoolExecutor(ORACLE_THREADS) as ex:
        return list(ex.map(fn, items))


# ---- presentations -----------------------------------------------------------------------------------------------------------

PRESENTATIONS = ("device-fixed", "device-ragged", "host-fixed", "host-ragged", "host-packed4")


def pack4_numpy(index_map: np.ndarray, reads2d: np.ndarray) -> np.ndarray:
    """ZSW_ENCODING_PACKED4 as include/zoe_sw.h words it: index_map[byte], the first base of a pair in the low nibble"""
    n, L = reads2d.shape
    idx = np.zeros((n, (L + 1) // 2 * 2), dtype=np.uint8)
    idx[:, :L] = np.asarray(index_map, dtype=np.uint8)[reads2d]
    return (idx[:, 0::2] | (idx[:, 1::2] << 4)).astype(np.uint8).reshape(-1)


class Presented:
    """A zsw_batch and the arrays it points to."""

    def __init__(self, _lib, rs: ReadSet, pres: str, lib=None, h=None, index_map=None, poison: bool = True):
        import torch

        self.rs, self.pres, self.device = rs, pres, pres.startswith("device")
        b = _lib.ZswBatch()
        b.n_reads, b.mem, b.encoding = rs.n, (_lib.MEM_DEVICE if self.device else _lib.MEM_HOST), 0
        fixed = pres.endswith("fixed") or pres.endswith("packed4")
        if fixed:
            assert rs.fixed_len > 0, "a ragged set has no fixed-length presentation"
        b.fixed_len = rs.fixed_len if fixed else 0
        self.keep = []
        bases = rs.bases
        if pres == "host-packed4":
            L = rs.fixed_len
            packed = np.full(rs.n * ((L + 1) // 2), FILL, dtype=np.uint8)
            assert lib.zsw_pack4_host(h, bases.ctypes.data, rs.n, L, packed.ctypes.data) == 0
            assert np.array_equal(packed, pack4_numpy(index_map, bases[: rs.n * L].reshape(rs.n, L))), "zsw_pack4_host differs from the numpy packer"
            if poison and L % 2:  # the unused high nibble of each read's last byte must not matter
                packed.reshape(rs.n, -1)[:, -1] |= 0xF0
            bases = packed
            b.encoding = 1
        offs = None if fixed else rs.offsets
        if self.device:
            tb = torch.from_numpy(bases).cuda()
            self.keep.append(tb)
            b.bases = tb.data_ptr()
            if offs is not None:
                to = torch.from_numpy(offs.astype(np.int64)).cuda()
                self.keep.append(to)
                b.offsets = to.data_ptr()
            torch.cuda.synchronize()
        else:
            self.keep.append(bases)
            b.bases = bases.ctypes.data
            if offs is not None:
                self.keep.append(offs)
                b.offsets = offs.ctypes.data
        self.batch = b

    def ref(self):
        return C.byref(self.batch)


# ---- output arrays with guards -----------------------------------------------------------------------------------------------

class Out:
    """n entries of `dtype` with GUARD entries in front and behind, all bytes FILL, in host or device memory"""

    def __init__(self, n: int, dtype, device: bool):
        self.n, self.dtype, self.device = n, np.dtype(dtype), device
        self.buf = np.full((n + 2 * GUARD) * self.dtype.itemsize, FILL, dtype=np.uint8)
        if device:
            import torch

            self.t = torch.from_numpy(self.buf).cuda()
            self.ptr = self.t.data_ptr() + GUARD * self.dtype.itemsize
        else:
            self.ptr = self.buf.ctypes.data + GUARD * self.dtype.itemsize

    def fetch(self) -> np.ndarray:
        raw = self.t.cpu().numpy() if self.device else self.buf
        return raw.view(self.dtype)

    def guards_intact(self) -> bool:
        raw = (self.t.cpu().numpy() if self.device else self.buf).reshape(self.n + 2 * GUARD, self.dtype.itemsize)
        return bool((raw[:GUARD] == FILL).all() and (raw[GUARD + self.n:] == FILL).all())

    def data(self) -> np.ndarray:
        return self.fetch()[GUARD:GUARD + self.n].copy()

    def untouched(self) -> bool:
        raw = self.t.cpu().numpy() if self.device else self.buf
        return bool((raw == FILL).all())


# ---- the entry points --------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Entry:
    name: str            # the C symbol
    kind: str            # "score" | "ends" | "ranges" | "align"
    cascade: bool        # the _from form: (from_width, preset_bits) and an out_tier array
    shared: bool
    threepass: bool = False

    @property
    def invert(self) -> int:
        return 1 if self.shared else 0  # SeqSrc::Query(read) is the usual call of the shared role

    def arrays(self):
        a = {"score": ["score"], "ends": ["score", "ref_end", "query_end"], "ranges": ["score", "ref_start", "ref_end", "query_start", "query_end"],
             "align": ["aln"]}[self.kind] + ["status"]
        return a + (["tier"] if self.cascade else [])


def _entries():
    out = []
    for shared in (False, True):
        s = "_shared" if shared else ""
        out += [
            Entry(f"zsw_score{s}_batch", "score", False, shared), Entry(f"zsw_score{s}_batch_from", "score", True, shared),
            Entry(f"zsw_score_ends{s}_batch", "ends", False, shared),
            Entry(f"zsw_score_ranges{s}_batch", "ranges", False, shared), Entry(f"zsw_score_ranges{s}_batch_from", "ranges", True, shared),
            Entry(f"zsw_align{s}_batch", "align", False, shared), Entry(f"zsw_align{s}_batch_from", "align", True, shared),
            Entry(f"zsw_align_3pass{s}_batch", "align", False, shared, True), Entry(f"zsw_align_3pass{s}_batch_from", "align", True, shared, True),
        ]
    return out


ENTRIES = _entries()
ENTRY = {e.name: e for e in ENTRIES}
DTYPES = {"score": np.uint32, "ref_end": np.uint32, "query_end": np.uint32, "ref_start": np.uint32, "query_start": np.uint32,
          "status": np.uint8, "tier": np.uint8, "aln": ALN_DTYPE, "inc": np.uint32, "op": np.uint8}


def stream_ptr(stream):
    return None if stream is None else C.c_void_p(stream.cuda_stream)


def _sync(stream, device: bool):
    if device:
        import torch

        (stream.synchronize() if stream is not None else torch.cuda.synchronize())


class Call:
    """One call of an entry point on a presented batch: allocates guarded outputs, issues the call (the alignment entry points
    through the ciglet capacity protocol), and keeps the result arrays. `launch()` only queues a device call; `collect()`
    synchronises and reads the arrays."""

    def __init__(self, _lib, lib, h, entry: Entry, p: Presented, stream=None, T: Optional[str] = None, lanes: Optional[int] = None,
                 from_width: int = 8, preset: int = 256):
        self._lib, self.lib, self.h, self.e, self.p, self.stream = _lib, lib, h, entry, p, stream
        self.n = p.rs.n
        self.a1, self.a2 = (from_width, preset) if entry.cascade else (_lib.INT_TYPES[T or p.rs.T], lanes or p.rs.lanes)
        self.out = {k: Out(self.n, DTYPES[k], p.device) for k in entry.arrays()}
        self.total = C.c_uint64(0)
        self.fn = getattr(lib, entry.name)
        self.rc = None

    def _args(self, inc_ptr=None, op_ptr=None, cap=0):
        o, e = self.out, self.e
        a = [self.h, self.p.ref(), self.a1, self.a2]
        if e.kind == "score":
            a += [o["score"].ptr, o["status"].ptr]
        elif e.kind == "ends":
            a += [o["score"].ptr, o["ref_end"].ptr, o["query_end"].ptr, o["status"].ptr]
        elif e.kind == "ranges":
            a += [o["score"].ptr, o["ref_start"].ptr, o["ref_end"].ptr, o["query_start"].ptr, o["query_end"].ptr, o["status"].ptr]
        else:
            a += [e.invert, o["aln"].ptr, o["status"].ptr]
        if e.cascade:
            a.append(o["tier"].ptr)
        if e.kind == "align":
            a += [inc_ptr, op_ptr, cap, C.byref(self.total)]
        return a + [stream_ptr(self.stream)]

    def launch(self):
        """score / ends / ranges: the one call (asynchronous for device batches)"""
        assert self.e.kind != "align"
        self.rc = self.fn(*self._args())
        return self

    def run_align(self):
        """capacity 0 with null arrays -> INVALID_ARGUMENT and the total; total - 1 the same, nothing written; total succeeds"""
        e, o, dev = self.e, self.out, self.p.device
        msg = lambda: self.lib.zsw_last_error_string(self.h).decode()
        rc0 = self.fn(*self._args(None, None, 0))
        t = int(self.total.value)
        if t == 0:
            assert rc0 == 0, (rc0, msg())
        else:
            assert rc0 == -1 and "capacity" in msg(), (rc0, msg())
            _sync(self.stream, dev)
            assert all(a.guards_intact() for a in o.values()), "guard entries changed by a call that failed for capacity"
        o["inc"], o["op"] = Out(t, np.uint32, dev), Out(t, np.uint8, dev)
        if t > 0:
            self.total.value = 0
            rc1 = self.fn(*self._args(o["inc"].ptr, o["op"].ptr, t - 1))
            assert rc1 == -1 and int(self.total.value) == t and "capacity" in msg(), (rc1, self.total.value, t, msg())
            _sync(self.stream, dev)
            assert all(a.guards_intact() for a in o.values()), "guard entries changed by a call that failed for capacity"
        self.total.value = 0
        self.rc = self.fn(*self._args(o["inc"].ptr, o["op"].ptr, t))
        assert int(self.total.value) == t, (self.total.value, t)
        return self

    def run(self):
        return self.run_align() if self.e.kind == "align" else self.launch()

    def collect(self) -> dict:
        assert self.rc == 0, (self.e.name, self.rc, self.lib.zsw_last_error_string(self.h).decode())
        _sync(self.stream, self.p.device)
        res = {}
        for k, a in self.out.items():
            assert a.guards_intact(), f"{self.e.name}: guard entries around `{k}` were written"
            res[k] = a.data()
        assert not (res["status"] == FILL).any(), f"{self.e.name}: statuses of some reads were never written"
        if self.e.kind == "align":
            res["total"] = np.array([self.total.value], dtype=np.uint64)
        return res


def assert_same(got: dict, want: dict, what: str):
    assert got.keys() == want.keys(), what
    for k in want:
        if not np.array_equal(got[k], want[k]):
            bad = np.nonzero(got[k] != want[k])[0] if got[k].shape == want[k].shape else []
            raise AssertionError(f"{what}: array `{k}` differs at {len(bad)} entries, first {list(bad[:5])}: got {got[k][bad[:5]]}, want {want[k][bad[:5]]}")


def aln_key(res: dict, i: int):
    """(status, score, ref range, query range, CIGAR, ref_len, query_len) as oracle.Aln.key()"""
    st = int(res["status"][i])
    if st != S_:
        return (st, 0, (0, 0), (0, 0), "", 0, 0)
    r = res["aln"][i]
    o, n = int(r["ciglet_offset"]), int(r["n_ciglets"])
    cigar = "".join(f"{int(res['inc'][o + k])}{chr(int(res['op'][o + k]))}" for k in range(n))
    return (st, int(r["score"]), (int(r["ref_start"]), int(r["ref_end"])), (int(r["query_start"]), int(r["query_end"])), cigar,
            int(r["ref_len"]), int(r["query_len"]))


def new_context(_lib, lib, matrix, go: int, ge: int, ref: Optional[bytes], pseq: Optional[bytes] = None):
    h = C.c_void_p()
    assert lib.zsw_create(0, C.byref(h)) == 0
    w = np.ascontiguousarray(matrix.signed_weights(), dtype=np.int8)
    im = np.ascontiguousarray(matrix.mapping.index_map, dtype=np.uint8)
    assert lib.zsw_set_scoring(h, w.ctypes.data, w.shape[0], im.ctypes.data, go, ge) == 0
    if ref is not None:
        r = np.frombuffer(ref, dtype=np.uint8)
        assert lib.zsw_set_reference(h, r.ctypes.data, len(ref), _lib.MEM_HOST) == 0
    if pseq is not None:
        p = np.frombuffer(pseq, dtype=np.uint8)
        assert lib.zsw_set_profile_sequence(h, p.ctypes.data, len(pseq), _lib.MEM_HOST) == 0
    return h
