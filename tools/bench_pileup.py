"""What piling alignments up costs (zsw_pileup_batch, include/zoe_sw.h): n synthetic 150-base reads on the device against a 2 kb
reference, zsw_align_3pass_batch_from, then the pile-up call over its records, everything device-resident, through the bare C ABI.
Timed in the same run, as yardsticks: the 3-pass call that produced the records and the stats-only zsw_annotate_batch call, which
walks the same records beside the same bases. Per call: the median of the timed steps and their min..max spread (host clocks around
a call that ends in a device synchronise, as tools/bench_annotate.py) and the bytes the call has to move per read, computed from the
shapes. Three cells: the bench's read set (reads that resemble the reference: the range route carries nearly every column), reads
that differ from the reference by 5 % (the per-column route carries more), and the bench's reads cut from a 30 kb reference (beyond
PILEUP_LDS_SITES_MAX: every add goes to the global workspace). Before a cell is timed its table is checked on the device against the
annotate stats of the same records: bins 0..4, 6 and 7 sum to matches + mismatches, the gap bin to del_bases, the insertion table to
ins_bases and ins_runs. zsw_consensus_from_counts on the 2 kb table is timed too.

Not measured: host batches (staged, bound by the copies), ragged batches, the role swap (ZSW_ANNOTATE_READ_IS_REF).

    python tools/bench_pileup.py [--reads 10000000] [--steps 7] [--warmup 2] [--out profiles/pileup_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

L = 150


def summary(times):
    return {"median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times)}


def timed(fn, steps, warmup):
    times = []
    for step in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if step >= warmup:
            times.append(time.perf_counter() - t0)
    return summary(times)


def cell(ctx, ref, rb, args):
    """align, check the table against the annotate stats, time the three calls -> the cell's record"""
    lib, h = ctx.lib, ctx.h
    n, R = rb.n_reads, len(ref)
    ctx.set_reference(ref)
    b = rb.c_batch()
    dev = rb.bases.device
    aln = torch.zeros(n * 10, dtype=torch.int32, device=dev)  # zsw_alignment: 40 bytes
    status, tier = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    total = C.c_uint64(0)
    cap = 4 * n
    while True:
        inc, op = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)

        def align():
            return lib.zsw_align_3pass_batch_from(h, C.byref(b), 8, 256, 0, aln.data_ptr(), status.data_ptr(), tier.data_ptr(), inc.data_ptr(), op.data_ptr(), cap,
                                                  C.byref(total), None)

        rc = align()
        if rc == -1 and total.value > cap:
            cap = int(total.value)
            continue
        ctx.check(rc)
        break
    t_in = int(total.value)
    stats = torch.zeros(n * 8, dtype=torch.int32, device=dev)  # zsw_alignment_stats: 32 bytes
    counts = torch.zeros((R, 8), dtype=torch.int32, device=dev)
    ins = torch.zeros((R + 1, 2), dtype=torch.int32, device=dev)
    n_bad = C.c_uint64(0)

    def annotate():
        return lib.zsw_annotate_batch(h, C.byref(b), 0, aln.data_ptr(), status.data_ptr(), inc.data_ptr(), op.data_ptr(), t_in, stats.data_ptr(), None, None, None, 0,
                                      None, None)

    def pileup(with_ins=True):
        return lib.zsw_pileup_batch(h, C.byref(b), 8, aln.data_ptr(), status.data_ptr(), inc.data_ptr(), op.data_ptr(), t_in, counts.data_ptr(),
                                    ins.data_ptr() if with_ins else None, C.byref(n_bad), None)  # 8: ZSW_PILEUP_CLEAR

    ctx.check(annotate())
    ctx.check(pileup())
    torch.cuda.synchronize()
    # the identities, on the device
    s = stats.view(n, 8).to(torch.int64)
    some = status == 0
    c, i = counts.to(torch.int64), ins.to(torch.int64)
    assert n_bad.value == 0, "a record of the alignment call is malformed"
    assert bool((s[:, 7][some] == 0).all()), "a SOME record did not walk to ZSW_PATH_OK"
    columns, gaps = int(c.sum() - c[:, 5].sum()), int(c[:, 5].sum())
    assert columns == int((s[:, 0] + s[:, 1]).sum()), "bins 0..4, 6, 7 != matches + mismatches"
    assert gaps == int(s[:, 3].sum()), "gap bin != del_bases"
    assert int(i[:, 1].sum()) == int(s[:, 2].sum()) and int(i[:, 0].sum()) == int(s[:, 4].sum()), "insertion table != ins_bases / ins_runs"
    mism = int(s[:, 1].sum())
    covered = int((c[:, :5].sum(dim=1) > 0).sum())
    del s, c, i
    # bytes the call has to move, from the shapes: the bases, the record, the status and the ciglets of every read once; per block
    # nothing per read is written. The tables (32 R + 8 (R + 1) bytes) and the workspace (16 (R + 1)) are read and written once more.
    nbytes = n * (L + 40 + 1) + 5 * t_in + 2 * (32 * R + 8 * (R + 1) + 16 * (R + 1))
    out = {"ref_len": R, "reads": n, "reads_with_alignment": int(some.sum()), "ciglets_in": t_in, "columns": columns, "mismatching_columns": mism,
           "gap_bases": gaps, "sites_covered": covered, "bytes": nbytes, "bytes_per_read": nbytes / n}
    out["zsw_align_3pass_batch_from"] = timed(align, args.steps, args.warmup)
    out["annotate_stats_only"] = timed(annotate, args.steps, args.warmup)
    out["pileup"] = timed(pileup, args.steps, args.warmup)
    out["pileup_without_insertion_table"] = timed(lambda: pileup(False), args.steps, args.warmup)
    out["pileup"]["fraction_of_align_call"] = out["pileup"]["median_ms"] / out["zsw_align_3pass_batch_from"]["median_ms"]
    out["pileup"]["fraction_of_annotate_call"] = out["pileup"]["median_ms"] / out["annotate_stats_only"]["median_ms"]
    out["pileup"]["bytes_per_s"] = nbytes / (1e-3 * out["pileup"]["median_ms"])
    if R <= 4096:
        fb = torch.from_numpy(__import__("numpy").frombuffer(ref, dtype="uint8").copy()).to(dev)
        seq = torch.empty(R, dtype=torch.uint8, device=dev)
        out["consensus_from_counts"] = timed(lambda: lib.zsw_consensus_from_counts(h, counts.data_ptr(), R, 1, 1, fb.data_ptr(), seq.data_ptr(), None), args.steps, args.warmup)
        out["consensus_differs_from_reference_at"] = int((seq != fb).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pileup.py needs a GPU"
    import zoe_amd
    from zoe_amd import synth

    n = args.reads
    ctx = zoe_amd.SwContext.get(0)
    ctx.set_scoring(zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N"), -10, -1)
    ref2k, ref30k = synth.reference_host(2000), synth.reference_host(30000)
    result = {"read_len": L, "steps": args.steps, "warmup": args.warmup,
              "timing": "host clock around a call that ends in a device synchronise; median and min..max of the timed steps",
              "not_measured": ["host batches", "ragged batches", "the role swap (ZSW_ANNOTATE_READ_IS_REF)"]}
    result["bench_reads_2kb"] = cell(ctx, ref2k, synth.reads_device(ctx, ref2k, 0, n, L), args)
    torch.cuda.empty_cache()
    result["diverged_5pct_2kb"] = cell(ctx, ref2k, synth.diverged_reads_device(ctx, ref2k, n, L, 0.05), args)
    torch.cuda.empty_cache()
    result["bench_reads_30kb"] = cell(ctx, ref30k, synth.reads_device(ctx, ref30k, 0, n, L), args)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
