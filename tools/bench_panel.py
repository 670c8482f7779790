"""Panel score call against the K-call recipe: n reads of 150 bases, device-resident, against a panel of 8 random members of 900 to
2,400 bases, the reads drawn evenly from the members (interleaved). Three sets — the members' reads at the bench's divergence (1 %
substitutions, 0.1 % + 0.1 % indels, 0.5 % N, 2 % random reads), the same at 5 % + 0.5 %, all random.

Each set is timed three ways, alternating within every step so that the ways see the same machine:
  panel    zsw_score_panel_batch_from (sw_score_panel_from_i8)
  recipe   what a caller did before: per member set_reference + sw_score_from_i8 on the whole batch; the per-read selection (rank,
           lowest member, in torch) is timed separately and is NOT part of "recipe"
  plain    sw_score_from_i8 of member 0's own reads (an eighth of the batch) against member 0 alone: what a caller who knows the
           member pays, for scale
Times are host clocks around work that ends in a device synchronise; per way the median of the steps and their min..max spread.
The results of `panel` and of the recipe + selection are compared read by read before anything is timed.

    python tools/bench_panel.py [--reads 10000000] [--steps 7] [--warmup 2] [--out FILE.json]
    python tools/bench_panel.py --only-panel 4        the first set, four panel calls and nothing else (under a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import zoe_amd
from zoe_amd import synth

K = 8


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def select(per_member):
    """the contract's ranking on the device: OVERFLOWED > SOME by score > UNMAPPED = EMPTY, ties to the lowest member"""
    def rank(s):
        score = s.score.to(torch.int64) & 0xFFFFFFFF
        return torch.where(s.status == 1, torch.full_like(score, 2 << 32), torch.where(s.status == 0, score | (1 << 32), torch.zeros_like(score)))

    best, score, status = rank(per_member[0]), per_member[0].score.clone(), per_member[0].status.clone()
    ref = torch.zeros_like(score)
    for k in range(1, len(per_member)):
        r = rank(per_member[k])
        better = r > best
        best = torch.where(better, r, best)
        score = torch.where(better, per_member[k].score, score)
        status = torch.where(better, per_member[k].status, status)
        ref = torch.where(better, torch.full_like(ref, k), ref)
    return score, status, ref


def interleave(parts, L):
    """reads of K equal parts, one of each in turn"""
    per = parts[0].n_reads
    stacked = torch.stack([p.bases[:per * L].reshape(per, L) for p in parts], dim=1)
    return zoe_amd.ReadBatch.from_fixed(stacked.reshape(-1).contiguous(), L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-panel", type=int, default=0, metavar="N", help="the first set only: N panel calls and nothing else (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_panel.py needs a GPU"
    L = 150
    per = args.reads // K
    n = per * K
    ctx = zoe_amd.SwContext.get(0)
    rng = np.random.default_rng(20261021)
    members = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(rng.integers(900, 2401)))].tobytes() for _ in range(K)]
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    ctx.set_scoring(dna, -10, -1)
    ctx.set_panel(members)
    idx = torch.randint(0, 4, (n * L,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    random_bases = 65 + 2 * (idx == 1).to(torch.uint8) + 6 * (idx == 2).to(torch.uint8) + 19 * (idx == 3).to(torch.uint8)  # A C G T
    del idx
    own = [synth.reads_device(ctx, m, k * per, per, L) for k, m in enumerate(members)]
    if args.only_panel:
        prof = zoe_amd.LocalProfilesBatch.new_with_w256(interleave(own, L), dna, -10, -1)
        for _ in range(args.only_panel):
            prof.sw_score_panel_from_i8()
            torch.cuda.synchronize()
        print(ctx.panel_counts())
        return
    sets = {
        "resembling (1 % + 0.2 %)": interleave(own, L),
        "resembling (5 % + 0.5 %)": interleave([synth.diverged_reads_device(ctx, m, per, L, 0.05, seed=20261021 + k) for k, m in enumerate(members)], L),
        "all random": zoe_amd.ReadBatch.from_fixed(random_bases, L),
    }
    plain_prof = zoe_amd.LocalProfilesBatch.new_with_w256(own[0], dna, -10, -1)
    result = {"reads": n, "read_len": L, "member_lens": [len(m) for m in members], "steps": args.steps, "warmup": args.warmup, "sets": {}}
    for name, rb in sets.items():
        prof = zoe_amd.LocalProfilesBatch.new_with_w256(rb, dna, -10, -1)
        recipe = lambda: [prof.sw_score_from_i8(m) for m in members]
        # results first: the new call against the recipe and the selection
        got = prof.sw_score_panel_from_i8()
        counts = ctx.panel_counts()
        ws, wst, wref = select(recipe())
        torch.cuda.synchronize()
        assert torch.equal(got.score, ws) and torch.equal(got.status, wst) and torch.equal(got.ref, wref), f"{name}: results differ from the recipe's"
        del got, ws, wst, wref
        t = {k: [] for k in ("panel", "recipe", "select", "plain")}
        for step in range(args.warmup + args.steps):
            row = {}
            row["panel"], _ = timed(prof.sw_score_panel_from_i8)
            row["recipe"], per_member = timed(recipe)
            row["select"], _ = timed(lambda: select(per_member))
            row["plain"], _ = timed(lambda: plain_prof.sw_score_from_i8(members[0]))
            del per_member
            if step >= args.warmup:
                for k, v in row.items():
                    t[k].append(v)
        summary = {k: {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v)} for k, v in t.items()}
        summary["settled"] = counts[0] / n
        summary["pairs_per_read"] = (counts[1] + counts[2]) / n
        summary["counts"] = list(counts)
        result["sets"][name] = summary
        print(f"{name}: settled after one score {counts[0]} ({100 * counts[0] / n:.2f} %), pairs scored {counts[1]} + {counts[2]} "
              f"({(counts[1] + counts[2]) / n:.3f} per read of {K}), scored against every member {counts[3]}")
        for k in ("panel", "recipe", "select", "plain"):
            s = summary[k]
            reads = per if k == "plain" else n
            print(f"  {k:8s} {s['median_ms']:9.2f} ms  ({s['min_ms']:.2f} .. {s['max_ms']:.2f})  {reads / s['median_ms'] / 1e3:8.1f} M reads/s", flush=True)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
