"""A call's result does not depend on what the context did before.

A zsw_context keeps state between calls: the staging and workspace buffers only grow (and keep the tails of larger calls), the
k-mer indices of the reference and of the profile sequence are built lazily and rebuilt after a change of sequence or matrix, and
the last-call record says whether the counters behind zsw_prune_rescored / zsw_min_score_counts belong to the last call. What a
call decides for itself (its target, the passes its batch takes, its result arrays) travels in values of that call, not on the
context. One long-lived context runs a fixed list of calls in which each pair that could leak stands next to each other (large then small, fixed then ragged, host then device, shared then read role,
option and debug bits on then off, a long reference then the short one, a 25-letter matrix then DNA, debug records on then off, a
failing call then a good one — also one that fails inside a shared-role call —, certificate alignment / 3-pass / certificate
alignment, a shared seeded pass directly before a read-role seeded reverse pass). After every call the same call is made on
a context created for it, and every output array and zsw_prune_rescored must be equal. No oracle here: test_gpu_abi_matrix.py
and the rest of the suite tie the results of a fresh context to it."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah
from abi_helpers import ENTRY

pytestmark = pytest.mark.gpu

DEFAULTS = dict(matrix=None, ref=None, pseq=None, pruning=1, debug=0, band=False, cert=False)

# (changes of the context's configuration, failing call made first on the long-lived context or None, entry point, batch, presentation)
STEPS = [
    (dict(matrix="dna", ref="short"), None, "zsw_score_batch_from", "big", "host-fixed"),
    ({}, None, "zsw_score_batch_from", "small", "host-fixed"),            # large then small: stale tails of the workspaces
    ({}, None, "zsw_score_batch_from", "ragged_small", "host-ragged"),    # fixed then ragged
    ({}, None, "zsw_score_batch_from", "ragged_small", "device-ragged"),  # host then device
    ({}, None, "zsw_score_ends_batch", "big", "host-fixed"),
    ({}, None, "zsw_score_ends_batch", "ragged_small", "device-ragged"),
    ({}, None, "zsw_score_ranges_batch_from", "big", "device-fixed"),
    ({}, None, "zsw_score_ranges_batch_from", "ragged_small", "host-ragged"),
    ({}, None, "zsw_align_batch_from", "big", "host-fixed"),              # alignment with certificates ...
    ({}, None, "zsw_align_batch_from", "small", "device-fixed"),
    ({}, None, "zsw_align_3pass_batch_from", "small", "host-fixed"),      # ... then 3-pass ...
    ({}, None, "zsw_align_batch_from", "small", "host-fixed"),            # ... then alignment again
    (dict(pseq="other"), None, "zsw_score_shared_batch_from", "big", "host-fixed"),  # a profile sequence of another length than the reference
    ({}, None, "zsw_score_batch_from", "small", "host-fixed"),            # shared role then read role ...
    ({}, None, "zsw_score_ranges_shared_batch", "small", "device-fixed"),  # ... and back
    ({}, None, "zsw_score_ranges_batch", "small", "host-fixed"),
    ({}, None, "zsw_align_shared_batch_from", "small", "host-fixed"),
    ({}, None, "zsw_score_ends_batch", "small", "host-packed4"),
    ({}, None, "zsw_score_ends_shared_batch", "ragged_small", "host-ragged"),
    ({}, None, "zsw_align_3pass_shared_batch_from", "small", "device-fixed"),
    ({}, None, "zsw_align_batch_from", "ragged_small", "device-ragged"),
    (dict(pruning=0), None, "zsw_score_batch_from", "big", "device-fixed"),   # ZSW_OPTION_EXACT_PRUNING 0 (frees the workspace) ...
    (dict(pruning=1), None, "zsw_score_batch_from", "big", "device-fixed"),   # ... then 1
    (dict(debug="any_size"), None, "zsw_score_ranges_batch_from", "few", "host-fixed"),  # seeded pass below 1,024 reads ...
    (dict(debug=0), None, "zsw_score_ranges_batch_from", "few", "host-fixed"),           # ... then the full pass
    (dict(ref="long"), None, "zsw_score_batch_from", "long_ref", "host-fixed"),    # >= 8,192 bases: handed-back reads in row chunks
    ({}, None, "zsw_align_batch_from", "long_ref", "device-fixed"),
    (dict(ref="short"), None, "zsw_score_batch_from", "small", "host-fixed"),      # the short reference again
    ({}, None, "zsw_score_ranges_batch_from", "small", "device-fixed"),
    (dict(matrix="protein", ref="protein", debug="any_size"), None, "zsw_score_batch_from", "protein", "device-fixed"),  # column-pruned pass
    ({}, None, "zsw_score_batch", "protein", "host-fixed"),
    (dict(matrix="dna", ref="short", debug=0), None, "zsw_score_batch_from", "small", "host-fixed"),  # DNA again
    ({}, None, "zsw_align_3pass_batch", "small", "host-fixed"),
    (dict(band=True), None, "zsw_score_batch_from", "small", "device-fixed"),      # zsw_debug_band_records on ...
    ({}, None, "zsw_score_ranges_batch_from", "small", "device-fixed"),
    (dict(band=False), None, "zsw_score_batch_from", "small", "device-fixed"),     # ... and off
    (dict(cert=True), None, "zsw_align_batch_from", "small", "host-fixed"),        # zsw_debug_cert_records on ...
    (dict(cert=False), None, "zsw_align_batch_from", "small", "device-fixed"),     # ... and off
    ({}, "bad_lanes", "zsw_score_batch", "small", "host-fixed"),                    # a failing call directly before a good one
    ({}, "offsets", "zsw_score_batch_from", "ragged_small", "host-ragged"),
    ({}, "capacity", "zsw_align_batch_from", "small", "host-fixed"),
    ({}, None, "zsw_score_batch_from", "big", "host-fixed"),
    ({}, "shared_offsets", "zsw_score_batch_from", "ragged_small", "host-ragged"),  # a shared-role call that fails while its batch is staged
    ({}, "shared_capacity", "zsw_align_batch_from", "small", "host-fixed"),         # ... and one that fails when it delivers
    ({}, None, "zsw_score_ends_shared_batch", "small", "device-fixed"),             # a shared seeded pass ...
    ({}, None, "zsw_score_ranges_batch_from", "small", "device-fixed"),             # ... then the read role's seeded reverse pass
]


@pytest.fixture(scope="module")
def world():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib, synth

    class W:
        pass

    w = W()
    w.za, w._lib, w.lib = zoe_amd, _lib, _lib.load()
    w.dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    short, long_ = synth.reference_host(2000), synth.reference_host(9000, seed=7)
    # a 25-letter matrix and residues (the column-pruned pass; as in __graft_entry__.smoke)
    keys = b"ACDEFGHIKLMNPQRSTVWYBJZX*"
    rng = np.random.default_rng(5)
    pw = rng.integers(-4, 3, size=(25, 25))
    pw = np.minimum(pw, pw.T)
    np.fill_diagonal(pw, rng.integers(4, 12, size=25))
    w.protein = zoe_amd.WeightMatrix.new_custom(zoe_amd.ByteIndexMap.new(keys, b"X"), pw.astype(np.int8))
    alpha = np.frombuffer(keys[:20], dtype=np.uint8)
    pref = rng.choice(alpha, 900).astype(np.uint8)
    start = rng.integers(0, 900 - 120, size=2000)
    preads = pref[start[:, None] + np.arange(120)[None, :]].copy()
    preads[rng.random(preads.shape) < 0.04] = alpha[3]
    preads[::7] = rng.choice(alpha, (len(preads[::7]), 120))
    w.refs = {"short": short, "long": long_, "protein": pref.tobytes()}
    w.pseqs = {"other": synth.reference_host(1200, seed=9)}
    w.matrices = {"dna": (w.dna, -10, -1), "protein": (w.protein, -11, -1)}
    w.sets = {
        "big": ah.mixed_set("big", short, 20000, 150, 1),
        "small": ah.mixed_set("small", short, 1500, 151, 2),
        "few": ah.mixed_set("few", short, 600, 150, 3),
        "ragged_small": ah.mixed_set("ragged_small", short, 1500, 0, 4),
        "long_ref": ah.mixed_set("long_ref", long_, 3000, 150, 5),
        "protein": ah.ReadSet("protein", w.refs["protein"], [bytes(r) for r in preads], 120, np.zeros(2000, dtype=np.int64), np.full(2000, -1)),
    }
    w.records = {}
    return w


def _records(w, who, kind, per_read):
    """zeroed device memory for the debug records of up to 20,000 reads, one buffer per context (`who`) and kind"""
    import torch

    if (who, kind) not in w.records:
        w.records[(who, kind)] = torch.zeros(per_read * 20000, dtype=torch.int32, device="cuda")
    return w.records[(who, kind)].data_ptr()


def configure(w, h, who, old, new):
    """brings context h from configuration `old` to `new` through the configuration calls, touching only what differs"""
    lib, _lib = w.lib, w._lib
    if new["matrix"] != old["matrix"]:
        m, go, ge = w.matrices[new["matrix"]]
        wt = np.ascontiguousarray(m.signed_weights(), dtype=np.int8)
        im = np.ascontiguousarray(m.mapping.index_map, dtype=np.uint8)
        assert lib.zsw_set_scoring(h, wt.ctypes.data, wt.shape[0], im.ctypes.data, go, ge) == 0
    if new["ref"] != old["ref"]:
        r = np.frombuffer(w.refs[new["ref"]], dtype=np.uint8)
        assert lib.zsw_set_reference(h, r.ctypes.data, len(r), _lib.MEM_HOST) == 0
    if new["pseq"] != old["pseq"]:
        p = np.frombuffer(w.pseqs[new["pseq"]], dtype=np.uint8)
        assert lib.zsw_set_profile_sequence(h, p.ctypes.data, len(p), _lib.MEM_HOST) == 0
    if new["pruning"] != old["pruning"]:
        assert lib.zsw_set_option(h, _lib.OPTION_EXACT_PRUNING, new["pruning"]) == 0
    if new["debug"] != old["debug"]:
        assert lib.zsw_debug_set(h, _lib.DEBUG_SCORE_PRUNE_ANY_SIZE if new["debug"] == "any_size" else 0) == 0
    if new["band"] != old["band"]:
        assert lib.zsw_debug_band_records(h, _records(w, who, "band", 8) if new["band"] else None) == 0
    if new["cert"] != old["cert"]:
        assert lib.zsw_debug_cert_records(h, _records(w, who, "cert", 4) if new["cert"] else None) == 0


def fail_first(w, h, kind, p):
    """a call that fails, on a context that must answer the next call as if it had not happened"""
    lib, _lib, n = w.lib, w._lib, p.rs.n
    score, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    msg = lambda: lib.zsw_last_error_string(h).decode()
    if kind == "bad_lanes":
        assert lib.zsw_score_batch(h, p.ref(), 1, 3, score.ctypes.data, status.ctypes.data, None) == -1 and "lanes" in msg()
    elif kind in ("offsets", "shared_offsets"):
        bad = p.rs.offsets.copy()
        bad[n // 2] = bad[n // 2 + 1] + 40  # goes backwards after this entry, inside the buffer
        b = _lib.ZswBatch()
        b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem = p.rs.bases.ctypes.data, bad.ctypes.data, 0, n, _lib.MEM_HOST
        fn = lib.zsw_score_batch_from if kind == "offsets" else lib.zsw_score_shared_batch_from
        assert fn(h, C.byref(b), 8, 256, score.ctypes.data, status.ctypes.data, None, None) == -1 and "monotone" in msg()
    elif kind in ("capacity", "shared_capacity"):
        aln = np.zeros(n, dtype=ah.ALN_DTYPE)
        inc, op, total = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8), C.c_uint64(0)
        fn, invert = (lib.zsw_align_batch_from, 0) if kind == "capacity" else (lib.zsw_align_shared_batch_from, 1)
        rc = fn(h, p.ref(), 8, 256, invert, aln.ctypes.data, status.ctypes.data, None, inc.ctypes.data, op.ctypes.data, 1, C.byref(total), None)
        assert rc == -1 and total.value > 1 and "capacity" in msg()
    else:
        raise AssertionError(kind)


def rescored(w, h):
    v = C.c_uint64(0)
    assert w.lib.zsw_prune_rescored(h, C.byref(v)) == 0
    return int(v.value)


def test_results_do_not_depend_on_the_contexts_history(world):
    w = world
    lib, _lib = w.lib, w._lib
    old = C.c_void_p()
    assert lib.zsw_create(0, C.byref(old)) == 0
    state = dict(DEFAULTS)
    presented = {}
    witnesses = set()
    try:
        for k, (changes, failing, entry_name, set_name, pres) in enumerate(STEPS):
            what = f"step {k}: {entry_name} {set_name} {pres} after {changes or 'no change'}{' and a failing call' if failing else ''}"
            new = dict(state, **changes)
            configure(w, old, "old", state, new)
            state = new
            if (set_name, pres) not in presented:  # (packed4: the DNA matrix is set when the one packed step comes)
                m = w.matrices[state["matrix"]][0]
                presented[(set_name, pres)] = ah.Presented(_lib, w.sets[set_name], pres, lib, old, m.mapping.index_map)
            p = presented[(set_name, pres)]
            T, lanes = ("i16", 16)
            if failing:
                fail_first(w, old, failing, p)
            got = ah.Call(_lib, lib, old, ENTRY[entry_name], p, None, T, lanes).run().collect()
            got_back = rescored(w, old)
            fresh = C.c_void_p()
            assert lib.zsw_create(0, C.byref(fresh)) == 0
            try:
                configure(w, fresh, "fresh", DEFAULTS, state)
                want = ah.Call(_lib, lib, fresh, ENTRY[entry_name], p, None, T, lanes).run().collect()
                want_back = rescored(w, fresh)
            finally:
                lib.zsw_destroy(fresh)
            ah.assert_same(got, want, what)
            assert got_back == want_back, (what, got_back, want_back)
            if got_back:
                witnesses.add((state["matrix"], state["ref"]))
        # the list did take the paths it names: the seeded pass on both references and the column-pruned pass handed reads back
        assert witnesses >= {("dna", "short"), ("dna", "long"), ("protein", "protein")}, witnesses
    finally:
        lib.zsw_destroy(old)
