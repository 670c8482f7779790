"""The whole launch sequence of a score call, route by route.

Other tests assert that a certain record is, or is not, in zsw_debug_score_launches. Here every call's FULL list of
(kind, G, C, mode) records is held to tests/golden/score_launch_sequences.json, which was recorded from the library as it was
before the score dispatcher (zsw_score.hip: launch_score / launch_score_rev; zsw_score_seed.hip: launch_score_seeded) was split into
steps with explicit streams, and is kept unchanged: a host-side restructuring must leave every sequence as it is (the module
passes on that earlier library and on the split one). The cases together reach every
note_launch site of those two files (the union of the golden's kinds covers every ZSW_LAUNCH_* name the sources hold), and every
call's result arrays are compared with the oracle as tests/test_gpu_seed_thresholds.py does — caller-owned arrays filled with
0xA5 through the C ABI, every read checked — so that a case cannot pass with the right launches and wrong answers.

Reads: the junk / clean / arrival reads of tests/test_gpu_seed_thresholds.py and tests/test_gpu_coschedule.py on their 300-base
reference, at 150 and 153 bases; a ragged pool of 24 to 400 bases on the same reference; reads beyond the widest strip
configuration (2,432 columns) on a 300-base reference (so that the cases under ZSW_DEBUG_NO_TILES, which walk a read per thread,
stay short); the tiled reads of tests/strip_edge_reads.py whose scores leave the packed range (4,600-base reference), and a smaller
batch of the same kind for the repeat under ZSW_DEBUG_NO_W32, where the exact kernel walks the worklist; world A of
tests/chunk_edge_reads.py (8,193 rows: the row-chunked full pass); 120-residue reads over 25 letters built by
test_gpu_strip_edges.fixed_edge_reads. No case holds more than 4,200 reads.

Recording (from a build whose sequences are the reference):  python tests/test_gpu_launch_sequences.py --record [PATH]
runs the cases of this module — oracle comparisons included — and writes the sequences to PATH (default: the golden file)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import abi_helpers as ah
import chunk_edge_reads as cer
import strip_edge_reads as ser
import test_gpu_seed_thresholds as st
import test_gpu_strip_edges as se

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "score_launch_sequences.json")
RECORD_ENV = "ZSW_RECORD_LAUNCH_SEQUENCES"  # set by --record: the path the sequences are written to
SOURCES = ("zsw_score.hip", "zsw_score_seed.hip")
MAX_READS = 4200
BELOW = 4  # ZSW_STATUS_BELOW_MIN_SCORE
L150, L153, L_LONG = 150, 153, 2500
N_JUNK = 129
DNA, DNA_W32 = (2, -5, -10, -1), se.SCHEMES[2]  # (5, -4, -120, -100): re-based every 64 rows, packed limit 16,952
DNA_W32_SMALL = (27, -4, -120, -100)             # the same gaps and limit: 628 matches leave the packed range
PROT_SCHEME = se.WIDE_SCHEMES[0]


def _flags():
    from zoe_amd import _lib as L

    return L


# ---- contexts: name -> (matrix kind of test_gpu_strip_edges.matrix, scheme, reference) ---------------------------------------------
def ref300(alpha=b"ACGT"):
    return np.frombuffer(alpha, np.uint8)[np.random.default_rng(300).integers(0, len(alpha), st.REF_LEN)]


def reference_of(name):
    if name == "ref300":
        return ref300().tobytes()
    if name == "prot300":
        return ref300(se.PROT).tobytes()
    if name == "prot900":
        return ser.reference(se.PROT)[:900]
    if name == "edges":
        return ser.reference()
    if name == "edges700":
        return ser.reference()[:700]
    assert name == "chunksA"
    return cer.world("A").ref


CONTEXTS = {
    "dna": ("dna", DNA, "ref300"),
    "dna-all": ("dna-all", DNA, "ref300"),
    "dna-w32": ("dna", DNA_W32, "edges"),
    "dna-w32-small": ("dna", DNA_W32_SMALL, "edges700"),
    "dna-chunks": ("dna", cer.WORLDS["A"][0], "chunksA"),
    "prot": ("prot", PROT_SCHEME, "prot900"),
    "prot-long": ("prot", PROT_SCHEME, "prot300"),
}


# ---- pools of distinct reads, batches as index arrays into them ---------------------------------------------------------------------
class Pool:
    def __init__(self, reads):
        self.reads = [bytes(r) for r in reads]  # distinct reads, as bytes
        self.want = {}                          # (context, kind) -> the oracle's results, per distinct read


def pool_fixed(length):
    """test_gpu_coschedule's pool: junk (no 8-mer of the reference), clean copies, and at 150 bases the arrivals"""
    ref = ref300()
    present = np.zeros(4 ** st.K, dtype=bool)
    present[st._kmer_codes(ref[None, :])[0]] = True
    cand = ah.ACGT[np.random.default_rng(4321).integers(0, 4, (14000, L153))]
    junk = cand[~present[st._kmer_codes(cand)].any(axis=1)][:N_JUNK, :length]
    assert len(junk) == N_JUNK
    parts = [junk, np.stack([ref[s:s + length] for s in range(st.REF_LEN - length + 1)])]
    if length == L150:
        parts.append(np.stack([np.concatenate([ref[s:s + st.GAP_AT], ref[s + st.GAP_AT + st.GAP:s + length + st.GAP]]) for s in range(st.REF_LEN - length - st.GAP + 1)]))
    p = Pool([r.tobytes() for part in parts for r in part])
    p.clean0, p.n_clean = N_JUNK, len(parts[1])
    p.arr0, p.n_arr = N_JUNK + len(parts[1]), len(parts[2]) if length == L150 else 0
    return p


def pool_ragged():
    """24 to 400 bases on the 300-base reference: per length copies (of the reference twice over), diverged copies and random reads"""
    rng = np.random.default_rng(24400)
    ref = ref300()
    ref2 = np.concatenate([ref, ref])
    reads = []
    for length in (24, 50, 76, 77, 100, 150, 152, 153, 200, 304, 305, 400):
        for k in range(20):
            reads.append(ref2[k * 13:k * 13 + length].tobytes())
        for k in range(6):
            reads.append(ah._substitute(rng, ref2[k * 31:k * 31 + length], 0.08).tobytes())
            reads.append(ah.ACGT[rng.integers(0, 4, length)].tobytes())
    return Pool(reads)


def pool_long(alpha, junk):
    """Reads beyond the widest strip configuration, on the 300-base reference of the alphabet. The first five have 2,500 bases (the
    fixed batch): the reference over and over, a 20-base copy that ends in the last column of tile 0, one that starts in the first
    of tile 1, a random read, the whole reference between junk. Then 2,433, 2,600 and 5,000 bases, and some short reads."""
    A = np.frombuffer(alpha, np.uint8)
    rng = np.random.default_rng(2433)
    ref = ref300(alpha).tobytes()
    T = ser.TILE_COLS
    fit = lambda b, n: (b + junk * n)[:n]
    reads = [fit(ref * 9, L_LONG), fit(junk * (T - 20) + ref[100:120], L_LONG), fit(junk * T + ref[100:120], L_LONG),
             A[rng.integers(0, len(A), L_LONG)].tobytes(), fit(junk * 1000 + ref, L_LONG),
             fit(ref * 9, T + 1), fit(junk * 100 + ref[100:120] + junk * T + ref[100:120], 2600), fit(ref * 17, 5000)]
    reads += [ref[s:s + 150] for s in range(0, 100, 10)] + [fit(ref + ref, 400), fit(ref[7:] + ref, 399)]
    return Pool(reads)


def pool_prot():
    ref = reference_of("prot900")
    return Pool([r.tobytes() for r in se.fixed_edge_reads(ref, 120, 4, 30, 300, se.PROT, b"X", seed=120)])


def pool_w32():
    """the reads of test_gpu_strip_edges beyond every strip configuration: under DNA_W32 the copies of 4,864 and 4,900 bases score
    beyond the packed range"""
    ref = reference_of("edges")
    reads = ser.edge_reads(ref)
    tiled = len(ser.length_classes())
    return Pool([r.seq for r in reads if r.cls == tiled])


def pool_w32_small():
    """The same route at a size the exact kernel (a read per thread, a third of a microsecond per cell: 7 s for the two reads above
    under ZSW_DEBUG_NO_W32) walks in half a second: a 700-base reference, a match of 27, and 2,433-base reads that hold the whole
    reference (18,900, beyond the packed range), half of it, or a piece in either tile."""
    ref = reference_of("edges700")
    n = ser.TILE_COLS + 1
    return Pool([b"N" * (n - 700) + ref, ref + b"N" * (n - 700), b"N" * 1000 + ref[:350] + b"N" * (n - 1350), ref[100:120] + b"N" * (n - 40) + ref[300:320]])


def pool_chunks():
    cs = cer.world("A").classes[0]
    p = Pool([r.tobytes() for r in cs.pool])
    p.cs = cs
    return p


POOLS = {"p150": lambda: pool_fixed(L150), "p153": lambda: pool_fixed(L153), "ragged": pool_ragged, "long": lambda: pool_long(b"ACGT", b"N"),
         "long-prot": lambda: pool_long(se.PROT, b"X"), "prot": pool_prot, "w32": pool_w32, "w32-small": pool_w32_small, "chunks": pool_chunks}


def batch_indices(name, p):
    """(pool, fixed length or 0, indices into the pool)"""
    cat = lambda *a: st.shuffled(np.concatenate(a).astype(np.int64))
    if name == "mix150":  # 129 junk (the seed kernel's hand-backs), 2,048 copies, 2,000 arrivals (fewer than 16,384: the second tier hands them back)
        return L150, cat(np.arange(N_JUNK), st.even_idx(p.clean0, p.n_clean, 2048), st.even_idx(p.arr0, p.n_arr, 2000))
    if name == "small150":
        return L150, cat(np.arange(N_JUNK), st.even_idx(p.clean0, p.n_clean, 600), st.even_idx(p.arr0, p.n_arr, 270))
    if name == "mix153":
        return L153, cat(np.arange(N_JUNK), st.even_idx(p.clean0, p.n_clean, 2048))
    if name == "ragged":
        return 0, cat(np.tile(np.arange(len(p.reads)), 8))
    if name == "long-fixed":
        return L_LONG, cat(np.tile(np.arange(5), 3))
    if name == "long-ragged":
        return 0, cat(np.arange(len(p.reads)), np.arange(len(p.reads)))
    if name == "prot":
        return 120, np.arange(len(p.reads))
    if name == "w32":
        return 0, np.arange(len(p.reads))
    if name == "w32-small":
        return ser.TILE_COLS + 1, np.arange(len(p.reads))
    assert name == "chunks"
    return L150, cer.batch_indices(p.cs, 101, 1024)


BATCHES = {"mix150": "p150", "small150": "p150", "mix153": "p153", "ragged": "ragged", "long-fixed": "long", "long-ragged": "long",
           "prot": "prot", "w32": "w32", "w32-small": "w32-small", "chunks": "chunks"}

SCORE, ENDS, RANGES, SHARED_ENDS = "zsw_score_batch_from", "zsw_score_ends_batch", "zsw_score_ranges_batch", "zsw_score_ends_shared_batch"


def cases():
    """name -> (context, batch, entry point, debug flags, ZSW_OPTION_MIN_SCORE: 0 off, 1 = the largest score of the junk reads, pool)"""
    L = _flags()
    ANY, STRIP = L.DEBUG_SCORE_PRUNE_ANY_SIZE, L.DEBUG_PRUNE_STRIP
    c = {}

    def add(name, ctx, batch, entry=SCORE, flags=0, min_score=0, pool=None):
        assert name not in c
        c[name] = (ctx, batch, entry, flags, min_score, pool or BATCHES[batch])

    add("plain", "dna", "small150")
    add("seeded", "dna", "mix150", flags=ANY)
    add("seeded-no-coschedule", "dna", "mix150", flags=ANY | L.DEBUG_SEED_NO_COSCHEDULE)
    add("seeded-strip-first-tier", "dna", "mix150", flags=ANY | L.DEBUG_SEED_STRIP_FIRST_TIER)
    add("seeded-wide-band", "dna", "mix150", flags=ANY | L.DEBUG_SEED_WIDE_BAND)
    add("seeded-no-band", "dna", "mix150", flags=ANY | L.DEBUG_SEED_NO_BAND)
    add("seeded-ends", "dna", "mix150", ENDS, ANY)
    add("seeded-ends-no-band", "dna", "mix150", ENDS, ANY | L.DEBUG_SEED_NO_BAND)
    add("seeded-153", "dna", "mix153", flags=ANY)
    add("min-score-seeded", "dna", "mix150", flags=ANY, min_score=1)
    add("min-score-plain", "dna", "small150", min_score=1)
    add("ragged", "dna", "ragged")
    add("ragged-seeded", "dna", "ragged", flags=ANY)
    add("ragged-seeded-no-side-streams", "dna", "ragged", flags=ANY | L.DEBUG_NO_SIDE_STREAMS)
    add("pruned-strip", "dna", "mix150", flags=ANY | STRIP)
    add("pruned-strip-ragged", "dna", "ragged", flags=ANY | STRIP)
    add("pruned-wide", "prot", "prot", flags=ANY)
    add("v1-fast", "dna", "small150", flags=L.DEBUG_SCORE_V1)
    add("v1-biased", "dna-all", "small150", flags=L.DEBUG_SCORE_V1)
    add("no-wide", "prot", "prot", flags=L.DEBUG_NO_WIDE)
    for ctx, pool, tag in (("dna", "long", "v2"), ("prot-long", "long-prot", "wide")):
        for batch in ("long-fixed", "long-ragged"):
            add(f"tiles-{tag}-{batch[5:]}", ctx, batch, pool=pool)
            add(f"tiles-{tag}-{batch[5:]}-no-tiles", ctx, batch, flags=L.DEBUG_NO_TILES, pool=pool)
    add("w32-worklist", "dna-w32", "w32")
    add("w32-small-worklist", "dna-w32-small", "w32-small")
    add("w32-small-worklist-no-w32", "dna-w32-small", "w32-small", flags=L.DEBUG_NO_W32)
    add("row-chunks", "dna-chunks", "chunks")
    add("row-chunks-off", "dna-chunks", "chunks", flags=L.DEBUG_NO_ROW_CHUNKS)
    add("ranges", "dna", "mix150", RANGES, ANY)
    add("ranges-exact-reverse", "dna", "mix150", RANGES, ANY | L.DEBUG_RANGES_EXACT_REVERSE)
    add("ranges-biased", "dna-all", "small150", RANGES)
    add("ranges-long", "dna", "long-fixed", RANGES)
    add("ranges-wide", "prot", "prot", RANGES)
    add("shared-ends", "dna", "mix150", SHARED_ENDS, ANY)
    return c


CASE_NAMES = ["plain", "seeded", "seeded-no-coschedule", "seeded-strip-first-tier", "seeded-wide-band", "seeded-no-band", "seeded-ends",
              "seeded-ends-no-band", "seeded-153", "min-score-seeded", "min-score-plain", "ragged", "ragged-seeded",
              "ragged-seeded-no-side-streams", "pruned-strip", "pruned-strip-ragged", "pruned-wide", "v1-fast", "v1-biased", "no-wide",
              "tiles-v2-fixed", "tiles-v2-fixed-no-tiles", "tiles-v2-ragged", "tiles-v2-ragged-no-tiles", "tiles-wide-fixed",
              "tiles-wide-fixed-no-tiles", "tiles-wide-ragged", "tiles-wide-ragged-no-tiles", "w32-worklist", "w32-small-worklist", "w32-small-worklist-no-w32",
              "row-chunks", "row-chunks-off", "ranges", "ranges-exact-reverse", "ranges-biased", "ranges-long", "ranges-wide", "shared-ends"]


# ---- the environment: contexts, pools and oracle results, built as the cases ask for them ------------------------------------------------
class Ctx:
    pass


class Env:
    def __init__(self, oracle):
        import zoe_amd
        from zoe_amd import _lib

        self.za, self._lib, self.lib, self.oracle = zoe_amd, _lib, _lib.load(), oracle
        self.ctx, self.pools, self.recorded = {}, {}, {}
        self.cases = cases()
        assert sorted(self.cases) == sorted(CASE_NAMES)

    def context(self, name):
        if name not in self.ctx:
            kind, scheme, ref_name = CONTEXTS[name]
            w = Ctx()
            w._lib, w.lib, w.oracle = self._lib, self.lib, self.oracle
            w.ref = reference_of(ref_name)
            m = se.matrix(self.za, kind, scheme)
            w.sc = self.oracle.Scoring(m.signed_weights(), m.mapping.index_map, scheme[2], scheme[3])
            w.h = ah.new_context(self._lib, self.lib, m, scheme[2], scheme[3], w.ref, pseq=w.ref)  # (the shared role's profile: the reference)
            self.ctx[name] = w
        return self.ctx[name]

    def pool(self, name):
        if name not in self.pools:
            self.pools[name] = POOLS[name]()
        return self.pools[name]

    def want(self, ctx_name, pool_name, entry):
        """the oracle's results for every distinct read of the pool, once per (context, entry point)"""
        w, p, o = self.context(ctx_name), self.pool(pool_name), self.oracle
        if (ctx_name, entry) not in p.want:
            if entry == SCORE:
                bases, off = ser.concat(p.reads)
                got = o.batch_score_w256(8, w.sc, bases, w.ref, offsets=off, threads=16)
            elif entry == ENDS:
                got = ser.oracle_map(lambda r: o.score_ends("i16", 16, w.sc, r, w.ref), p.reads)
            elif entry == SHARED_ENDS:
                got = ser.oracle_map(lambda r: o.score_ends("i16", 16, w.sc, w.ref, r), p.reads)
            else:
                got = ser.oracle_map(lambda r: o.score_ranges("i16", 16, w.sc, r, w.ref), p.reads)
            p.want[(ctx_name, entry)] = got
        return p.want[(ctx_name, entry)]

    def close(self):
        for w in self.ctx.values():
            self.lib.zsw_set_option(w.h, self._lib.OPTION_MIN_SCORE, C.c_int64(0))
            self.lib.zsw_debug_set(w.h, 0)
            self.lib.zsw_destroy(w.h)


@pytest.fixture(scope="module")
def env(oracle):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    e = Env(oracle)
    yield e
    e.close()
    path = os.environ.get(RECORD_ENV)
    if path:
        assert sorted(e.recorded) == sorted(CASE_NAMES), "a recording holds every case"
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(e.recorded[k])}' for k in CASE_NAMES) + "\n}\n")


def golden():
    with open(GOLDEN) as f:
        return {k: [tuple(r) for r in v] for k, v in json.load(f).items()}


def check_ranges(res, want, what):
    unscored = int((res["status"] == ah.FILL).sum())
    assert unscored == 0, (what, f"{unscored} reads were never scored: their statuses are still the caller's fill")
    stt = np.array([r[0] for r in want], dtype=np.uint8)
    assert np.array_equal(res["status"], stt), what
    some = stt == ah.S_
    cols = {"score": [r[1] for r in want], "ref_start": [r[2][0] for r in want], "ref_end": [r[2][1] for r in want],
            "query_start": [r[3][0] for r in want], "query_end": [r[3][1] for r in want]}
    for field, v in cols.items():
        v = np.array(v, dtype=np.uint32)
        bad = np.nonzero(some & (res[field] != v))[0]
        assert len(bad) == 0, (what, field, f"{len(bad)} reads differ, first {bad[:5]}: got {res[field][bad[:5]]}, want {v[bad[:5]]}")


def run_case(e, name):
    """The call of a case, its arrays held to the oracle -> the launch log"""
    ctx_name, batch, entry, flags, min_score, pool_name = e.cases[name]
    w, p = e.context(ctx_name), e.pool(pool_name)
    fixed_len, idx = batch_indices(batch, p)
    assert len(idx) <= MAX_READS, (name, len(idx))
    reads = [p.reads[i] for i in idx]
    assert all(len(r) == fixed_len for r in reads) or fixed_len == 0
    rs = ah.ReadSet(name, w.ref, reads, fixed_len, np.zeros(len(idx), dtype=np.int64), np.full(len(idx), -1))
    want = e.want(ctx_name, pool_name, entry)
    t_min = 0
    if min_score:  # not above any junk read's whole-read bound (the seed kernel still hands them all back), above most of their scores
        t_min = int(want[0][:N_JUNK].max())
    assert e.lib.zsw_debug_set(w.h, flags) == 0
    assert e.lib.zsw_set_option(w.h, e._lib.OPTION_MIN_SCORE, C.c_int64(t_min)) == 0
    try:
        res, _, log, _ = st.call(w, entry, rs, "device-fixed" if fixed_len else "device-ragged")
    finally:
        assert e.lib.zsw_set_option(w.h, e._lib.OPTION_MIN_SCORE, C.c_int64(0)) == 0
        assert e.lib.zsw_debug_set(w.h, 0) == 0
    if entry == SCORE:
        score, status, tier = (a[idx].copy() for a in want)
        if t_min:  # the option's contract applied to the oracle
            below = (status == ah.U_) | ((status == ah.S_) & (score < t_min))
            assert 0 < int(below.sum()) < len(idx)
            score[below], status[below], tier[below] = 0, BELOW, 0
        st.check_score(res, (score, status, tier), np.arange(len(idx)), name)
    elif entry in (ENDS, SHARED_ENDS):
        st.check_ends(res, [want[i] for i in idx], name)
    else:
        check_ranges(res, [want[i] for i in idx], name)
    return log


@pytest.mark.parametrize("name", CASE_NAMES)
def test_launch_sequence_of_a_route_is_the_recorded_one(env, name):
    log = run_case(env, name)
    print(f"{name}: {log}")
    if os.environ.get(RECORD_ENV):
        env.recorded[name] = [list(r) for r in log]
        return
    assert log == golden()[name], (name, "launch sequence differs from the recorded one", log, golden()[name])


def test_side_streams_carry_no_launch_decision():
    """ragged, seeded per class: on side streams and on the caller's stream alone the same launches in the same order"""
    g = golden()
    assert g["ragged-seeded-no-side-streams"] == g["ragged-seeded"] != g["ragged"]


def test_recorded_sequences_reach_every_launch_record_of_the_dispatcher():
    """every ZSW_LAUNCH_* name in zsw_score.hip and zsw_score_seed.hip is the kind of some record of the golden file"""
    L = _flags()
    names = set()
    for f in SOURCES:
        with open(os.path.join(ser.CSRC, f)) as src:
            names |= set(re.findall(r"\bZSW_(LAUNCH_[A-Z0-9_]+)\b", src.read()))
    assert len(names) >= 16, names
    kinds = {r[0] for seq in golden().values() for r in seq}
    missing = sorted(n for n in names if getattr(L, n) not in kinds)
    assert not missing, ("no recorded sequence holds a record of kind", missing)
    assert sorted(golden()) == sorted(CASE_NAMES)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_launch_sequences.py --record [PATH]")
    os.environ[RECORD_ENV] = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN
    sys.exit(pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "-s", "--durations=12", "-p", "no:cacheprovider",
                          "-k", "test_launch_sequence_of_a_route_is_the_recorded_one"]))
