"""What a minimum score buys (ZSW_OPTION_MIN_SCORE, include/zoe_sw.h): zsw_score_batch_from over n device-resident reads of 150
bases vs a 2 kb reference, for five read sets — the bench's own generator, 5 %, 8 % and 12 %-diverged reads of
tools/bench_divergence.py, all random — and T in {0, 150, 225, 250}. Per cell: the median of the timed steps and their min..max
spread (host clocks around a call that ends in a device synchronise, as tools/bench_strands.py), zsw_prune_rescored and the four
counters of zsw_min_score_counts. The all-random x T = 0 cell is the full pass over every read: the floor the others are read against.

"T = 0 costs nothing": with --parent-lib PATH (the library built from the parent commit) the bench set's T = 0 call is also timed
through the bare C ABI — the same few lines for both libraries, each in a process of its own, alternating — and both medians and
the parent's own min..max spread go into the JSON; a difference outside that spread is a regression.

    python tools/bench_min_score.py [--reads 10000000] [--steps 7] [--warmup 2] [--parent-lib PATH] [--out profiles/min_score_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

T_VALUES = (0, 150, 225, 250)
RATES = (5, 8, 12)


def summary(times):
    return {"median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times)}


def bare_abi(lib_path, n, steps, warmup):
    """zsw_score_batch_from (8 / 256) over the bench's reads through ctypes alone: entry points every version of the library has"""
    lib = C.CDLL(lib_path)
    vp = C.c_void_p
    lib.zsw_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.zsw_destroy.argtypes = [vp]
    lib.zsw_destroy.restype = None
    lib.zsw_set_scoring.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int]
    lib.zsw_set_reference.argtypes = [vp, vp, C.c_size_t, C.c_int]
    lib.zsw_synth_reference_host.argtypes = [C.c_uint64, C.c_uint64, vp]
    lib.zsw_synth_reference_host.restype = None
    lib.zsw_synth_reads.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp]

    class Batch(C.Structure):
        _fields_ = [("bases", vp), ("offsets", vp), ("fixed_len", C.c_uint32), ("n_reads", C.c_uint64), ("mem", C.c_int), ("encoding", C.c_int)]

    lib.zsw_score_batch_from.argtypes = [vp, C.POINTER(Batch), C.c_int, C.c_int, vp, vp, vp, vp]
    h = vp()
    assert lib.zsw_create(0, C.byref(h)) == 0
    im = np.full(256, 4, dtype=np.uint8)  # DNA_PROFILE_MAP: ACGTN, U = T, either case
    for i, ch in enumerate(b"ACGT"):
        im[ch] = im[ch + 32] = i
    im[ord("U")] = im[ord("u")] = 3
    w = np.full((5, 5), -5, dtype=np.int8)
    np.fill_diagonal(w, 2)
    w[4, :] = w[:, 4] = 0
    assert lib.zsw_set_scoring(h, w.ctypes.data, 5, im.ctypes.data, -10, -1) == 0
    ref = np.zeros(2000, dtype=np.uint8)
    lib.zsw_synth_reference_host(42, 2000, ref.ctypes.data)
    assert lib.zsw_set_reference(h, ref.ctypes.data, 2000, 0) == 0
    bases = torch.empty(n * 150, dtype=torch.uint8, device="cuda")
    assert lib.zsw_synth_reads(h, 1337, 0, n, 150, bases.data_ptr(), None) == 0
    score, status, tier = (torch.empty(n, dtype=t, device="cuda") for t in (torch.int32, torch.uint8, torch.uint8))
    b = Batch(bases.data_ptr(), None, 150, n, 1, 0)
    times = []
    for step in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert lib.zsw_score_batch_from(h, C.byref(b), 8, 256, score.data_ptr(), status.data_ptr(), tier.data_ptr(), None) == 0
        torch.cuda.synchronize()
        if step >= warmup:
            times.append(time.perf_counter() - t0)
    out = summary(times)
    out["checksum"] = int(score.to(torch.int64).sum()) + int(status.to(torch.int64).sum()) * 1_000_003
    lib.zsw_destroy(h)
    return out


def table(n, steps, warmup):
    import zoe_amd
    from zoe_amd import synth

    ctx = zoe_amd.SwContext.get(0)
    ref = synth.reference_host(2000)
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    L = 150

    def random_set():
        idx = torch.randint(0, 4, (n * L,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        return zoe_amd.ReadBatch.from_fixed(65 + 2 * (idx == 1).to(torch.uint8) + 6 * (idx == 2).to(torch.uint8) + 19 * (idx == 3).to(torch.uint8), L)

    makers = [("bench set", lambda: synth.reads_device(ctx, ref, 0, n, L))]
    makers += [(f"{r} % diverged", (lambda r=r: synth.diverged_reads_device(ctx, ref, n, L, r / 100.0))) for r in RATES]
    makers.append(("all random", random_set))
    sets = {}
    for name, make in makers:
        rb = make()
        prof = zoe_amd.LocalProfilesBatch.new_with_w256(rb, dna, -10, -1)
        base = prof.sw_score_from_i8(ref)
        cells = {}
        for t in T_VALUES:
            ctx.set_min_score(t)
            try:
                got = prof.sw_score_from_i8(ref)
                back, counts = ctx.prune_rescored(), ctx.min_score_counts()
                # the contract on the T = 0 results, before anything is timed
                below = ((base.status == 2) | ((base.status == 0) & (base.score < t))) if t else torch.zeros_like(base.status, dtype=torch.bool)
                ok = torch.equal(got.status, torch.where(below, torch.full_like(base.status, 4), base.status)) and \
                    torch.equal(got.score, torch.where(below, torch.zeros_like(base.score), base.score))
                assert ok and counts[3] == int(below.sum()), f"{name}, T = {t}: results differ from the contract"
                times = []
                for step in range(warmup + steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    prof.sw_score_from_i8(ref, out=got)
                    torch.cuda.synchronize()
                    if step >= warmup:
                        times.append(time.perf_counter() - t0)
            finally:
                ctx.set_min_score(0)
            cell = summary(times)
            cell.update({"zsw_prune_rescored": back, "counts": list(counts), "below_share": counts[3] / n, "settled_by_whole_read_bound": counts[0] / max(counts[3], 1),
                         "settled_by_band_bound": counts[1] / max(counts[3], 1), "settled_by_exact_score": counts[2] / max(counts[3], 1)})
            cells[f"T={t}"] = cell
            print(f"{name:14s} T {t:3d}: {cell['median_ms']:8.2f} ms ({cell['min_ms']:.2f} .. {cell['max_ms']:.2f})  rescored {back:9d}  counts {list(counts)}", flush=True)
        sets[name] = cells
        del rb, prof, base, got
        torch.cuda.empty_cache()
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bare-abi", default=None, help=argparse.SUPPRESS)  # child mode: time one library through the bare C ABI, print JSON
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_min_score.py needs a GPU"
    if args.bare_abi:
        print(json.dumps(bare_abi(args.bare_abi, args.reads, args.steps, args.warmup)))
        return
    result = {"reads": args.reads, "read_len": 150, "ref_len": 2000, "steps": args.steps, "warmup": args.warmup, "call": "zsw_score_batch_from (8 / 256), device-resident"}
    if args.parent_lib:
        from zoe_amd import _lib

        def child(path):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--bare-abi", path, "--reads", str(args.reads), "--steps", str(args.steps), "--warmup",
                                  str(args.warmup)], capture_output=True, text=True, check=True)
            return json.loads(out.stdout.strip().splitlines()[-1])

        runs = {"parent": [], "this": []}
        for _ in range(2):  # alternating, so that both see the same machine
            runs["parent"].append(child(os.path.abspath(args.parent_lib)))
            runs["this"].append(child(_lib.LIB_PATH))
        assert len({r["checksum"] for rs in runs.values() for r in rs}) == 1, "the two libraries computed different results"
        parent = min(runs["parent"], key=lambda r: r["median_ms"])
        this = min(runs["this"], key=lambda r: r["median_ms"])
        spread = parent["max_ms"] - parent["min_ms"]
        result["t0_costs_nothing"] = {"parent": runs["parent"], "this_commit_T0": runs["this"], "parent_median_ms": parent["median_ms"], "this_median_ms": this["median_ms"],
                                      "parent_spread_ms": spread, "difference_ms": this["median_ms"] - parent["median_ms"],
                                      "inside_parent_spread": this["median_ms"] - parent["median_ms"] <= spread}
        print("T = 0 against the parent's library (bare C ABI): " + json.dumps(result["t0_costs_nothing"]), flush=True)
    result["sets"] = table(args.reads, args.steps, args.warmup)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
