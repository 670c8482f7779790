"""Strand-aware score call against the two-call recipe: n reads of 150 bases vs a 2 kb reference, device-resident, three sets —
all forward (the bench's generator), half of them reverse complemented, all random.

Each set is timed three ways, alternating within every step so that the ways see the same machine:
  strands  zsw_score_strands_batch_from (sw_score_strands_from_i8)
  recipe   what a caller did before: sw_score_from_i8 on the reads, sw_score_from_i8 on a reverse-complemented copy; the copy
           (zsw_orient_batch on the device, kinder to the recipe than a host loop) and the per-read selection (torch.where) are
           timed separately and are NOT part of "recipe"
  plain    sw_score_from_i8 alone (what a caller who knows the strand pays)
Times are host clocks around work that ends in a device synchronise; per way the median of the steps and their min..max spread.
The results of `strands` and of the recipe + selection are compared read by read before anything is timed.

    python tools/bench_strands.py [--reads 10000000] [--steps 7] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import zoe_amd
from zoe_amd import synth


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def select(f, r):
    """the contract's ranking on the device: OVERFLOWED > SOME by score > UNMAPPED = EMPTY, ties to the forward strand"""
    def rank(s):
        score = s.score.to(torch.int64) & 0xFFFFFFFF
        return torch.where(s.status == 1, torch.full_like(score, 2 << 32), torch.where(s.status == 0, score | (1 << 32), torch.zeros_like(score)))

    rev = rank(r) > rank(f)
    return torch.where(rev, r.score, f.score), torch.where(rev, r.status, f.status), rev.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_strands.py needs a GPU"
    n, L = args.reads, 150
    ctx = zoe_amd.SwContext.get(0)
    ref = synth.reference_host(2000)
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    ctx.set_scoring(dna, -10, -1)
    ctx.set_reference(ref)
    forward = synth.reads_device(ctx, ref, 0, n, L)
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    alternate = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
    idx = torch.randint(0, 4, (n * L,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    random_bases = 65 + 2 * (idx == 1).to(torch.uint8) + 6 * (idx == 2).to(torch.uint8) + 19 * (idx == 3).to(torch.uint8)  # A C G T
    del idx
    sets = {
        "all forward": forward,
        "half reverse": ctx.orient(forward, alternate),
        "all random": zoe_amd.ReadBatch.from_fixed(random_bases, L),
    }
    result = {"reads": n, "read_len": L, "ref_len": len(ref), "steps": args.steps, "warmup": args.warmup, "sets": {}}
    for name, rb in sets.items():
        prof = zoe_amd.LocalProfilesBatch.new_with_w256(rb, dna, -10, -1)
        ways = {
            "strands": lambda: prof.sw_score_strands_from_i8(ref),
            "plain": lambda: prof.sw_score_from_i8(ref),
        }
        # results first: the new call against the recipe and the selection
        got = prof.sw_score_strands_from_i8(ref)
        counts = ctx.strand_counts()
        rcb = ctx.orient(rb, ones)
        f, r = prof.sw_score_from_i8(ref), zoe_amd.LocalProfilesBatch.new_with_w256(rcb, dna, -10, -1).sw_score_from_i8(ref)
        ws, wst, wstrand = select(f, r)
        torch.cuda.synchronize()
        assert torch.equal(got.score, ws) and torch.equal(got.status, wst) and torch.equal(got.strand, wstrand), f"{name}: results differ from the recipe's"
        del got, f, r, ws, wst, wstrand, rcb
        t = {k: [] for k in ("strands", "recipe", "plain", "copy", "select")}
        for step in range(args.warmup + args.steps):
            row = {}
            row["strands"], _ = timed(ways["strands"])
            row["copy"], rcb = timed(lambda: ctx.orient(rb, ones))
            prof_rc = zoe_amd.LocalProfilesBatch.new_with_w256(rcb, dna, -10, -1)
            row["recipe"], (f, r) = timed(lambda: (prof.sw_score_from_i8(ref), prof_rc.sw_score_from_i8(ref)))
            row["select"], _ = timed(lambda: select(f, r))
            row["plain"], _ = timed(ways["plain"])
            del rcb, prof_rc, f, r
            if step >= args.warmup:
                for k, v in row.items():
                    t[k].append(v)
        summary = {k: {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v)} for k, v in t.items()}
        summary["scored_twice"] = counts[2] / n
        summary["counts"] = list(counts)
        result["sets"][name] = summary
        print(f"{name}: settled forward {counts[0]}, settled reverse {counts[1]}, scored twice {counts[2]} ({100 * counts[2] / n:.2f} %), answered reverse {counts[3]}")
        for k in ("strands", "recipe", "plain", "copy", "select"):
            s = summary[k]
            print(f"  {k:8s} {s['median_ms']:9.2f} ms  ({s['min_ms']:.2f} .. {s['max_ms']:.2f})  {n / s['median_ms'] / 1e3:8.1f} M reads/s", flush=True)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
