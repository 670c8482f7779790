"""Every strip-kernel instantiation at its structural edges, and proof of which instantiation ran.

The score kernels are compiled once per strip configuration (G lanes per read pair, C columns per lane) and table form; random
reads reach most of them through a handful of reads and meet their geometric edges by luck. Here the edge reads of
tests/strip_edge_reads.py (checked against the oracle alone by tests/test_strip_edge_reads.py) go through every family of kernels —
score_kernel_v2, score_kernel with the four-entry and with the biased table, the LDS-table (WIDE) form, the reversed kernels of
the ranges calls, the tiled kernels, the seeded pass in front of them — under schemes that re-base the drift domain every 2,048,
1,024 and 64 rows or never. Every comparison is equality with the oracle, and zsw_debug_score_launches must show that the
instantiation meant did the work: a length class that quietly went to the exact 32-bit kernel would otherwise pass.

The oracle's results are computed once per weight matrix and scheme and shared by the tests (and families) that use that matrix.
The ends of sw_score_ends are those of the oracle's score_ranges: its forward pass is sw_simd_score_ends (striped.rs:361-364).
"""
import numpy as np
import pytest

import strip_edge_reads as ser

pytestmark = pytest.mark.gpu

S_ = 0
SCHEMES = [(2, -5, -10, -1), (6, -5, -12, -5), (5, -4, -120, -100), (3, -4, -5, 0)]  # re-base period 2,048 / 1,024 / 64 rows / none
WIDE_SCHEMES = [(0, 0, -11, -1), (0, 0, -14, -6)]  # (the 25-letter matrix is fixed; gap_extend 1 and 6)
PROT = b"ACDEFGHIKLMNPQRSTVWY"
PROT_KEYS = b"ACDEFGHIKLMNPQRSTVWYBJZX*"
TN = [("i16", 16), ("i16", 8)]  # the stripe order of the oracle's profile differs: ties among columns must not


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


@pytest.fixture
def ctx(za):
    """The context with its debug flags and options restored after the test."""
    from zoe_amd import _lib

    c = za.SwContext.get(0)
    yield c
    c.debug_set(0)
    c.set_option(_lib.OPTION_EXACT_PRUNING, 1)


# ---- matrices, reads and oracle results, once per module ----------------------------------------------------------------------
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def matrix(za, kind, scheme):
    """kind 'dna': new_dna_matrix(match, mismatch, ignoring N) — v2 by default, the four-entry table of v1; 'dna-all': no letter
    ignored, so N scores the mismatch (the biased table of v1); 'prot': 25 letters, X (the junk of the edge reads) scores 0."""
    ma, mi = scheme[0], scheme[1]
    if kind == "dna":
        return za.WeightMatrix.new_dna_matrix(ma, mi, b"N")
    if kind == "dna-all":
        return za.WeightMatrix.new_dna_matrix(ma, mi, None)
    rng = np.random.default_rng(31)
    mp = za.ByteIndexMap.new(PROT_KEYS, b"X")
    w = rng.integers(-4, 3, size=(25, 25))
    w = np.minimum(w, w.T)
    np.fill_diagonal(w, rng.integers(4, 12, size=25))
    x = mp.to_index(b"X"[0])
    w[x, :] = 0
    w[:, x] = 0
    return za.WeightMatrix.new_custom(mp, w.astype(np.int8))


def edge_set(kind):
    def make():
        alpha, junk = (PROT, b"X") if kind == "prot" else (b"ACGT", b"N")
        ref = ser.reference(alpha)
        return ref, ser.edge_reads(ref, alpha, junk)

    return cached(("reads", kind), make)


def selection(kind, longest):
    """Indices of the edge reads of at most `longest` bases (all of them: None)."""
    reads = edge_set(kind)[1]
    return [i for i, r in enumerate(reads) if longest is None or len(r.seq) <= longest]


def device_batch(za, kind, longest=None):
    reads = edge_set(kind)[1]
    return cached(("batch", kind, longest), lambda: za.ReadBatch.from_sequences([reads[i].seq for i in selection(kind, longest)]))


def scoring(za, oracle, kind, scheme):
    m = matrix(za, kind, scheme)
    return oracle.Scoring(m.signed_weights(), m.mapping.index_map, scheme[2], scheme[3])


def want_score(za, oracle, kind, scheme):
    ref, reads = edge_set(kind)
    sc = scoring(za, oracle, kind, scheme)
    return cached(("score", kind, scheme), lambda: ser.oracle_map(lambda r: oracle.score("i16", 16, sc, r.seq, ref), reads))


def want_w256(za, oracle, kind, scheme):
    ref, reads = edge_set(kind)
    sc = scoring(za, oracle, kind, scheme)
    bases, off = ser.concat([r.seq for r in reads])
    return cached(("w256", kind, scheme), lambda: oracle.batch_score_w256(8, sc, bases, ref, offsets=off, threads=16))


def want_ranges(za, oracle, kind, scheme, T, N):
    ref, reads = edge_set(kind)
    sc = scoring(za, oracle, kind, scheme)
    return cached(("ranges", kind, scheme, T, N), lambda: ser.oracle_map(lambda r: oracle.score_ranges(T, N, sc, r.seq, ref), reads))


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def host(t):
    return t.cpu().numpy()


def check_score(got, want, what, index=None):
    st, s = host(got.status), host(got.score).view(np.uint32)
    for k, i in enumerate(range(len(want)) if index is None else index):
        o_st, o_s = want[i]
        assert (int(st[k]), int(s[k]) if o_st == S_ else 0) == (o_st, o_s if o_st == S_ else 0), (what, i)


def check_w256(got, want, what, index=None):
    ws, wst, wt = want if index is None else (a[index] for a in want)
    assert np.array_equal(host(got.status), wst), what
    assert np.array_equal(host(got.score).view(np.uint32), ws), what
    assert np.array_equal(host(got.tier), wt), what


def check_ends(got, ranges, what, index=None):
    st, s, re_, qe = host(got.status), host(got.score), host(got.ref_end), host(got.query_end)
    for k, i in enumerate(range(len(ranges)) if index is None else index):
        o_st, o_s, o_rr, o_qr = ranges[i]
        assert int(st[k]) == o_st, (what, i)
        if o_st == S_:
            assert (int(s[k]), int(re_[k]), int(qe[k])) == (o_s, o_rr[1], o_qr[1]), (what, i)


def check_ranges(got, ranges, what, index=None):
    st, s = host(got.status), host(got.score)
    rs, re_, qs, qe = host(got.ref_start), host(got.ref_end), host(got.query_start), host(got.query_end)
    for k, i in enumerate(range(len(ranges)) if index is None else index):
        o_st, o_s, o_rr, o_qr = ranges[i]
        assert int(st[k]) == o_st, (what, i)
        if o_st == S_:
            assert (int(s[k]), (int(rs[k]), int(re_[k])), (int(qs[k]), int(qe[k]))) == (o_s, o_rr, o_qr), (what, i)


def require(log, kind, mode, cfgs, what):
    missing = [(g, c) for g, c in cfgs if (kind, g, c, mode) not in log]
    assert not missing, (what, "not launched:", missing, "log:", sorted(set(log)))


def families():
    from zoe_amd import _lib as L

    return {
        "v2": dict(matrix="dna", flags=0, kind=L.LAUNCH_V2, tile=L.LAUNCH_TILE_V2, rev=L.LAUNCH_V1_FAST_REV),
        # score_kernel has no tiled form — reads beyond the widest configuration are the exact 32-bit kernel's, one thread per read,
        # seconds per call at 5,000 bases — so its families get the reads of the nineteen classes only
        "v1-fast": dict(matrix="dna", flags=L.DEBUG_SCORE_V1, kind=L.LAUNCH_V1_FAST, tile=None, rev=L.LAUNCH_V1_FAST_REV),
        # (no letter ignored: fast_ok fails; v2_ok fails too unless gap_extend lifts N's mismatch to 0 or more, as 5 does for the
        # mismatch of -5 and 100 for -4 — two of the four schemes: the flag keeps every scheme on score_kernel)
        "v1-biased": dict(matrix="dna-all", flags=L.DEBUG_SCORE_V1, kind=L.LAUNCH_V1_BIASED, tile=None, rev=L.LAUNCH_V1_BIASED_REV),
        "wide": dict(matrix="prot", flags=0, kind=L.LAUNCH_WIDE, tile=L.LAUNCH_TILE_WIDE, rev=L.LAUNCH_WIDE_REV),
    }


CASES = [(f, s) for f in ("v2", "v1-fast", "v1-biased") for s in SCHEMES] + [("wide", s) for s in WIDE_SCHEMES]


# ---- the ragged batch: every length class of every family in one call, under 1,024 reads (the full pass takes it) ------------------
@pytest.mark.parametrize("family,scheme", CASES)
def test_ragged_edge_batch_runs_every_class_configuration(za, oracle, ctx, family, scheme):
    from zoe_amd import _lib as L

    fam = families()[family]
    kind, go, ge = fam["matrix"], scheme[2], scheme[3]
    ref, reads = edge_set(kind)
    longest = None if fam["tile"] is not None else ser.TILE_COLS
    index = selection(kind, longest)
    rb, m = device_batch(za, kind, longest), matrix(za, kind, scheme)
    classes = ser.length_classes()
    assert len(reads) < 1024
    ctx.debug_set(fam["flags"])

    def check_log(mode, what):
        log = ctx.debug_score_launches()
        require(log, fam["kind"], mode, classes, (family, what))
        if fam["tile"] is not None:  # three tiles for the reads beyond 4,864 columns
            assert log.count((fam["tile"], 64, 38, mode)) >= 3, (family, what, sorted(set(log)))
            assert not [r for r in log if r[0] == L.LAUNCH_EXACT32], (family, what, "a whole class went to the exact 32-bit kernel")
        else:
            assert not [r for r in log if r[0] in (L.LAUNCH_EXACT32, L.LAUNCH_TILE_W32)], (family, what, sorted(set(log)))
        return log

    p = za.StripedProfileBatch(rb, m, go, ge, "i16", 16)
    check_score(p.sw_score(ref), want_score(za, oracle, kind, scheme), (family, "sw_score"), index)
    check_log(0, "sw_score")
    check_w256(za.LocalProfilesBatch.new_with_w256(rb, m, go, ge).sw_score_from_i8(ref), want_w256(za, oracle, kind, scheme), (family, "from_i8"), index)
    log = check_log(0, "sw_score_from_i8")
    if family == "v2" and ge in (-5, -100):  # the longest copies score beyond the packed range of these schemes: 32-bit tiles
        assert (L.LAUNCH_TILE_W32, 64, 38, 0) in log, sorted(set(log))
    for T, N in TN:
        want = want_ranges(za, oracle, kind, scheme, T, N)
        p = za.StripedProfileBatch(rb, m, go, ge, T, N)
        check_ends(p.sw_score_ends(za.SeqSrc.Reference(ref)), want, (family, "ends", T, N), index)
        check_log(2, "sw_score_ends")
        got = p.sw_score_ranges(za.SeqSrc.Reference(ref))
        log = ctx.debug_score_launches()
        check_ranges(got, want, (family, "ranges", T, N), index)
        require(log, fam["kind"], 2, classes, (family, "forward pass of the ranges"))
        if fam["tile"] is not None:  # reads beyond every strip configuration: the reverse pass of the batch is the 32-bit tile kernel's
            assert (L.LAUNCH_TILE_W32, 64, 38, 2) in log, (family, sorted(set(log)))
        else:  # ... otherwise the reversed kernel of the longest read's configuration
            assert (fam["rev"], 64, 38, 2) in log, (family, sorted(set(log)))


def test_wide_alphabet_without_the_wide_kernels_is_the_exact_kernel(za, oracle, ctx):
    """ZSW_DEBUG_NO_WIDE: a 25-letter batch in one exact32_kernel launch, same results. That kernel walks a read per thread, a
    third of a microsecond per cell: the reads of up to 608 bases (the classes of 4, 8 and 16 lanes) keep a call under a second."""
    from zoe_amd import _lib as L

    scheme = WIDE_SCHEMES[0]
    ref, reads = edge_set("prot")
    index = selection("prot", 608)
    rb, m = device_batch(za, "prot", 608), matrix(za, "prot", scheme)
    ctx.debug_set(L.DEBUG_NO_WIDE)
    p = za.StripedProfileBatch(rb, m, scheme[2], scheme[3], "i16", 16)
    check_score(p.sw_score(ref), want_score(za, oracle, "prot", scheme), "exact sw_score", index)
    assert ctx.debug_score_launches() == [(L.LAUNCH_EXACT32, 0, 0, 0)]
    check_ends(p.sw_score_ends(za.SeqSrc.Reference(ref)), want_ranges(za, oracle, "prot", scheme, "i16", 16), "exact ends", index)
    assert ctx.debug_score_launches() == [(L.LAUNCH_EXACT32, 0, 0, 2)]
    check_w256(za.LocalProfilesBatch.new_with_w256(rb, m, scheme[2], scheme[3]).sw_score_from_i8(ref), want_w256(za, oracle, "prot", scheme), "exact from_i8", index)
    assert ctx.debug_score_launches() == [(L.LAUNCH_EXACT32, 0, 0, 0)]
    p8 = za.StripedProfileBatch(rb, m, scheme[2], scheme[3], "i16", 8)
    check_ranges(p8.sw_score_ranges(za.SeqSrc.Reference(ref)), want_ranges(za, oracle, "prot", scheme, "i16", 8), "exact ranges", index)
    assert ctx.debug_score_launches() == [(L.LAUNCH_EXACT32, 0, 0, 2), (L.LAUNCH_EXACT32, 0, 0, 2)]  # forward, then the prefixes reversed


# ---- mode 1 (score + reference end): the first pass of sw_align when no certificate pass runs (batches under 1,024 reads) -----------
@pytest.mark.parametrize("family,scheme", [(f, s) for f in ("v2", "v1-fast", "v1-biased") for s in (SCHEMES[0], SCHEMES[2])] + [("wide", WIDE_SCHEMES[0])])
def test_first_pass_of_sw_align_runs_mode_1_in_every_class(za, oracle, ctx, family, scheme):
    """The alignment's score and reference end are those of the ranges (sw_simd_align and sw_simd_score_ends share the row rule).
    The 8..32-letter launcher serves mode 1 with its mode 2 instantiation; the log says so."""
    from zoe_amd import _lib as L

    fam = families()[family]
    kind, go, ge = fam["matrix"], scheme[2], scheme[3]
    ref, reads = edge_set(kind)
    index = selection(kind, ser.TILE_COLS)
    rb, m = device_batch(za, kind, ser.TILE_COLS), matrix(za, kind, scheme)
    want = want_ranges(za, oracle, kind, scheme, "i16", 16)
    ctx.debug_set(fam["flags"])
    aln = za.StripedProfileBatch(rb, m, go, ge, "i16", 16).sw_align(za.SeqSrc.Reference(ref))
    log = ctx.debug_score_launches()
    require(log, fam["kind"], 2 if family == "wide" else 1, ser.length_classes(), (family, "first pass of sw_align"))
    assert not [r for r in log if r[0] in (L.LAUNCH_EXACT32, L.LAUNCH_SEED_WINDOW, L.LAUNCH_SEED_BAND)], log
    for k, i in enumerate(index):
        o_st, o_s, o_rr, o_qr = want[i]
        assert int(aln.status[k]) == o_st, (family, i)
        if o_st == S_:
            assert (int(aln.records[k]["score"]), int(aln.records[k]["ref_end"])) == (o_s, o_rr[1]), (family, i, reads[i].tag)


def test_launch_log_reports_the_count_and_writes_nothing_into_a_short_buffer(za, ctx):
    import ctypes as C

    ref, reads = edge_set("dna")
    m = matrix(za, "dna", SCHEMES[0])
    za.StripedProfileBatch([r.seq for r in reads[:40]], m, -10, -1, "i16", 16).sw_score(ref)
    log = ctx.debug_score_launches()
    assert len(log) >= 3  # three classes and the worklist launch
    n = C.c_uint32(0)
    buf = np.full(4 * len(log) + 4, 0xDEADBEEF, dtype=np.uint32)
    for cap in (0, 1, len(log) - 1):
        assert ctx.lib.zsw_debug_score_launches(ctx.h, C.c_void_p(buf.ctypes.data), cap, C.byref(n)) == 0
        assert n.value == len(log) and (buf == 0xDEADBEEF).all(), cap
    assert ctx.lib.zsw_debug_score_launches(ctx.h, C.c_void_p(buf.ctypes.data), len(log) + 1, C.byref(n)) == 0
    assert n.value == len(log) and [tuple(int(v) for v in buf[4 * k:4 * k + 4]) for k in range(len(log))] == log
    assert (buf[4 * len(log):] == 0xDEADBEEF).all()
    assert ctx.lib.zsw_debug_score_launches(ctx.h, None, 0, None) != 0  # out_n is required
    assert ctx.debug_score_launches() == log  # reading the log does not change it


# ---- the reverse pass: one ranges call per class, so that launch_score_rev picks each first-fit configuration in turn ---------------
@pytest.mark.parametrize("family,scheme", [(f, s) for f in ("v1-fast", "v1-biased") for s in SCHEMES] + [("wide", s) for s in WIDE_SCHEMES])
def test_reverse_pass_in_every_first_fit_configuration(za, oracle, ctx, family, scheme):
    from zoe_amd import _lib as L

    fam = families()[family]
    kind, go, ge = fam["matrix"], scheme[2], scheme[3]
    ref, reads = edge_set(kind)
    m = matrix(za, kind, scheme)
    want = want_ranges(za, oracle, kind, scheme, "i16", 16)
    classes = ser.length_classes()
    ctx.debug_set(fam["flags"] | L.DEBUG_RANGES_EXACT_REVERSE)
    for k, (G, C) in enumerate(classes):
        index = [i for i, r in enumerate(reads) if r.cls == k]
        p = za.StripedProfileBatch([reads[i].seq for i in index], m, go, ge, "i16", 16)
        check_ranges(p.sw_score_ranges(za.SeqSrc.Reference(ref)), want, (family, "ranges of class", G, C), index)
        log = ctx.debug_score_launches()
        assert (fam["kind"], G, C, 2) in log and (fam["rev"], G, C, 2) in log, (family, G, C, log)
        assert not [r for r in log if r[0] in (L.LAUNCH_EXACT32, L.LAUNCH_TILE_W32)], (family, G, C, log)
    # (8,19) and (32,5) are never first fit: their reversed instantiations are not reachable (nothing to assert)


# ---- the seeded pass in front of the same kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_seeded_pass_over_the_edge_batch_equals_the_full_pass(za, oracle, ctx, scheme):
    from zoe_amd import _lib as L

    go, ge = scheme[2], scheme[3]
    ref, reads = edge_set("dna")
    rb, m = device_batch(za, "dna"), matrix(za, "dna", scheme)
    classes = ser.length_classes()
    lp = za.LocalProfilesBatch.new_with_w256(rb, m, go, ge)
    p = za.StripedProfileBatch(rb, m, go, ge, "i16", 16)
    full = lp.sw_score_from_i8(ref)
    full_ends = p.sw_score_ends(za.SeqSrc.Reference(ref))
    assert not [r for r in ctx.debug_score_launches() if r[0] in (L.LAUNCH_SEED_WINDOW, L.LAUNCH_SEED_BAND)]
    for flags, kinds in ((L.DEBUG_SCORE_PRUNE_ANY_SIZE | L.DEBUG_SEED_NO_BAND, (L.LAUNCH_SEED_WINDOW,)),
                         (L.DEBUG_SCORE_PRUNE_ANY_SIZE, (L.LAUNCH_SEED_WINDOW, L.LAUNCH_SEED_BAND))):
        ctx.debug_set(flags)
        got = lp.sw_score_from_i8(ref)
        log = ctx.debug_score_launches()
        for mode, g, f, name in ((0, got, full, "score"), (2, p.sw_score_ends(za.SeqSrc.Reference(ref)), full_ends, "ends")):
            if mode == 2:
                log = ctx.debug_score_launches()
            missing = [(G, C) for G, C in classes if not any((kd, G, C, mode) in log for kd in kinds)]
            assert not missing, (name, "no seeded launch for", missing, sorted(set(log)))
            # the reads handed back: gated launches in the configurations the cost model picks for short and long lists
            assert [r for r in log if r[0] == L.LAUNCH_V2 and r[3] == mode], (name, sorted(set(log)))
            for field in ("score", "status") + (("tier",) if mode == 0 else ("ref_end", "query_end")):
                assert np.array_equal(host(getattr(g, field)), host(getattr(f, field))), (name, field, flags)
        check_w256(got, want_w256(za, oracle, "dna", scheme), "seeded from_i8")
        check_ranges(p.sw_score_ranges(za.SeqSrc.Reference(ref)), want_ranges(za, oracle, "dna", scheme, "i16", 16), ("seeded ranges", flags))
        ctx.debug_set(0)


# ---- fixed-length batches: the batch-size-aware choice, which alone picks (32,5) and (8,19) ---------------------------------------
def model_config(L, n):
    """score_config_for_batch (zsw_score.hip): the cheapest configuration that holds L columns, for n reads."""
    best, pick = 0.0, None
    for G, C in ser.strip_configs():
        if G * C < L:
            continue
        cost = (7.5 * C + 25.0) * max(2048.0, ((n + 1) // 2) * G / 64.0)
        if pick is None or cost < best * 0.97:
            best, pick = cost, (G, C)
    return pick


def fixed_edge_reads(ref, L, G, C, n, alpha, junk, seed):
    """n reads of L bases on the edges of configuration (G, C): copies, last lane, last column, lane boundaries, gaps across them,
    the same segment in two lanes, mutated copies — at varying reference positions."""
    rng = np.random.default_rng(seed)
    A = np.frombuffer(alpha, np.uint8)
    J = junk
    j = G // 2
    out = np.empty((n, L), dtype=np.uint8)
    span = len(ref) - 2 * L
    for i in range(n):
        s = int(rng.integers(L, L + span))
        t = i % 9
        if t == 0:
            r = ref[s:s + L]
        elif t == 1:  # the last lane that holds columns of the read
            r = J * ((L - 1) // C * C) + ref[s:s + C]
        elif t == 2:
            r = J * (L - 1) + ref[s:s + 1]
        elif t == 3:
            r = J * (j * C - 20) + ref[s:s + 20]
        elif t == 4:
            r = J * (j * C) + ref[s:s + 20]
        elif t == 5:
            r = J * (j * C - 33) + ref[s:s + 30] + ser._foreign(alpha, ref[s + 90:s + 96]) + ref[s + 30:s + 60]
        elif t == 6:
            r = ref[s:s + 29] + ref[s + 35:s + 64]
        elif t == 7:
            r = ref[s:s + 20] + J * C + ref[s:s + 20]
        else:
            b = np.frombuffer(ref[s:s + L], np.uint8).copy()
            hit = rng.random(L) < 0.06
            b[hit] = rng.choice(A, int(hit.sum()))
            r = b.tobytes()
        r = (r + J * L)[:L]
        out[i] = np.frombuffer(r, np.uint8)
    return out


# (L, n, exact pruning, configuration): small batches of short reads take (32,5); tens of thousands of 150-base reads take (8,19)
# once the seeded pass is switched off (ZSW_OPTION_EXACT_PRUNING = 0: every cell of every read) ...
FIXED = [(160, 7, 1, (32, 5)), (159, 257, 1, (32, 5)), (153, 1023, 1, (32, 5)), (100, 301, 1, (32, 5)),
         (152, 30001, 0, (8, 19)), (150, 40000, 0, (8, 19)), (115, 30001, 0, (8, 19))]
# ... and by default the seeded pass in the first-fit configuration, its hand-backs gated over (32,5) and (4,38): score_kernel_v2 only
FIXED_CASES = [(f,) + c for f in ("v2", "v1-fast", "v1-biased", "wide") for c in FIXED] + [("v2", 150, 30001, 1, (4, 38))]


@pytest.mark.parametrize("family,L,n,pruning,cfg", FIXED_CASES)
def test_fixed_length_batches_reach_the_batch_size_aware_configurations(za, oracle, ctx, family, L, n, pruning, cfg):
    import torch

    from zoe_amd import _lib as LIB

    fam = families()[family]
    kind = fam["matrix"]
    scheme = WIDE_SCHEMES[0] if family == "wide" else SCHEMES[0]
    go, ge = scheme[2], scheme[3]
    G, C = cfg
    seeded = bool(pruning) and n >= 1024
    if seeded:  # (4,38) is the first fit; the hand-backs of a short list go where the model sends 16,384 reads
        assert model_config(L, 16384) == (32, 5)
    else:
        assert model_config(L, n) == cfg
    alpha, junk = (PROT, b"X") if kind == "prot" else (b"ACGT", b"N")
    ref = ser.reference(alpha)[:900]
    rd = fixed_edge_reads(ref, L, G, C, n, alpha, junk, seed=L * 1000003 + n)
    m, sc = matrix(za, kind, scheme), scoring(za, oracle, kind, scheme)
    rb = za.ReadBatch.from_fixed(torch.from_numpy(rd.reshape(-1)).cuda(), L)
    ctx.debug_set(fam["flags"])
    ctx.set_option(LIB.OPTION_EXACT_PRUNING, pruning)
    got = za.LocalProfilesBatch.new_with_w256(rb, m, go, ge).sw_score_from_i8(ref)
    log = ctx.debug_score_launches()
    check_w256(got, oracle.batch_score_w256(8, sc, rd, ref, fixed_len=L, threads=16), (family, L, n))
    if seeded:
        assert any(r[0] in (LIB.LAUNCH_SEED_WINDOW, LIB.LAUNCH_SEED_BAND) and r[1:3] == (4, 38) for r in log), log
        assert (LIB.LAUNCH_V2, 32, 5, 0) in log, log  # (a list of up to 49,152 hand-backs; (4,38) again is for batches beyond that)
    else:
        assert [r for r in log if r[0] != LIB.LAUNCH_EXACT32_WORKLIST] == [(fam["kind"], G, C, 0)], log
    ends = za.StripedProfileBatch(rb, m, go, ge, "i16", 16).sw_score_ends(za.SeqSrc.Reference(ref))
    log = ctx.debug_score_launches()
    if not seeded:
        assert [r for r in log if r[0] != LIB.LAUNCH_EXACT32_WORKLIST] == [(fam["kind"], G, C, 2)], log
    index = list(range(0, n, max(1, n // 63)))
    st, s, re_, qe = host(ends.status), host(ends.score), host(ends.ref_end), host(ends.query_end)
    for i, (o_st, (o_s, o_re, o_qe)) in zip(index, ser.oracle_map(lambda i: oracle.score_ends("i16", 16, sc, rd[i], ref), index)):
        assert int(st[i]) == o_st, (family, i)
        if o_st == S_:
            assert (int(s[i]), int(re_[i]), int(qe[i])) == (o_s, o_re, o_qe), (family, i)
