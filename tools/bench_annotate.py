"""What annotating alignments costs (zsw_annotate_batch, include/zoe_sw.h): n synthetic 150-base reads on the device against a 2 kb
reference, zsw_align_3pass_batch_from, then the annotate call over its records — stats only, and stats + verbose CIGAR — everything
device-resident, through the bare C ABI. Per call: the median of the timed steps and their min..max spread (host clocks around a
call that ends in a device synchronise, as tools/bench_min_score.py), the bytes the call has to move per read (computed from the
shapes and the ciglet counts of this batch, below), and that traffic over the time as a fraction of the 6.29 TB/s a float4 copy
reaches on an MI355X. Before anything is timed the results are checked on the device: every SOME record walks to ZSW_PATH_OK with
path_score == score, and the counts add up to the ranges.

    python tools/bench_annotate.py [--reads 10000000] [--steps 7] [--warmup 2] [--out profiles/annotate_bench.json]
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

COPY_RATE = 6.29e12  # bytes/s, measured float4 copy on an MI355X
L, REF_LEN = 150, 2000


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_annotate.py needs a GPU"
    import zoe_amd
    from zoe_amd import synth

    n = args.reads
    ctx = zoe_amd.SwContext.get(0)
    lib, h = ctx.lib, ctx.h
    ref = synth.reference_host(REF_LEN)
    ctx.set_scoring(zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N"), -10, -1)
    ctx.set_reference(ref)
    rb = synth.reads_device(ctx, ref, 0, n, L)
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
    out_aln = torch.zeros(n * 10, dtype=torch.int32, device=dev)
    vtotal = C.c_uint64(0)

    def annotate(verbose, vcap, vinc, vop):
        return lib.zsw_annotate_batch(h, C.byref(b), 0, aln.data_ptr(), status.data_ptr(), inc.data_ptr(), op.data_ptr(), t_in, stats.data_ptr(),
                                      out_aln.data_ptr() if verbose else None, vinc.data_ptr() if verbose and vinc is not None else None,
                                      vop.data_ptr() if verbose and vop is not None else None, vcap, C.byref(vtotal) if verbose else None, None)

    rc = annotate(True, 0, None, None)  # the capacity protocol: the required size comes back
    t_out = int(vtotal.value)
    assert (rc == -1 and t_out > 0) or (rc == 0 and t_out == 0), (rc, t_out)
    vinc, vop = torch.empty(max(t_out, 1), dtype=torch.int32, device=dev), torch.empty(max(t_out, 1), dtype=torch.uint8, device=dev)
    ctx.check(annotate(True, t_out, vinc, vop))
    torch.cuda.synchronize()
    # the self-check of every CIGAR, on the device
    s, a = stats.view(n, 8).to(torch.int64), aln.view(n, 10).to(torch.int64)
    some = status == 0
    assert bool((s[:, 7][some] == 0).all()) and bool((s[:, 7][~some] == 7).all()), "a SOME record did not walk to ZSW_PATH_OK"
    assert bool((s[:, 6][some] == a[:, 0][some]).all()), "path_score != score"
    assert bool(((s[:, 0] + s[:, 1] + s[:, 2])[some] == (a[:, 4] - a[:, 3])[some]).all()) and bool(((s[:, 0] + s[:, 1] + s[:, 3])[some] == (a[:, 2] - a[:, 1])[some]).all())
    n_some = int(some.sum())
    edits = {"mismatches": int(s[:, 1].sum()), "ins_bases": int(s[:, 2].sum()), "del_bases": int(s[:, 3].sum())}
    del s, a

    # bytes a call has to move, from the shapes: the count launch reads the bases, the record, the status and the ciglets of a read
    # and writes its stats; with a verbose CIGAR it also writes a count, the scan reads the counts and writes the starts, and the write
    # launch reads everything again (stats: the status word) and the two starts of a read, and writes a record and the verbose ciglets
    count_bytes = n * (L + 40 + 1 + 32) + 5 * t_in
    verbose_bytes = count_bytes + n * 8 + n * 16 + n * (L + 40 + 4 + 16 + 40) + 5 * t_in + 5 * t_out
    r_align = timed(align, args.steps, args.warmup)
    r_stats = timed(lambda: annotate(False, 0, None, None), args.steps, args.warmup)
    r_verbose = timed(lambda: annotate(True, t_out, vinc, vop), args.steps, args.warmup)
    for r, nbytes in ((r_stats, count_bytes), (r_verbose, verbose_bytes)):
        r["bytes_per_read"] = nbytes / n
        r["bytes"] = nbytes
        r["fraction_of_copy_rate"] = nbytes / (1e-3 * r["median_ms"]) / COPY_RATE
        r["fraction_of_align_call"] = r["median_ms"] / r_align["median_ms"]
    result = {"reads": n, "read_len": L, "ref_len": REF_LEN, "steps": args.steps, "warmup": args.warmup, "copy_rate_bytes_per_s": COPY_RATE,
              "timing": "host clock around a call that ends in a device synchronise; median and min..max of the timed steps",
              "reads_with_alignment": n_some, "ciglets_in": t_in, "ciglets_verbose": t_out, "edits": edits,
              "zsw_align_3pass_batch_from": r_align, "annotate_stats_only": r_stats, "annotate_stats_and_verbose": r_verbose}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
