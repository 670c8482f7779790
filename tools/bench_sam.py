"""What formatting SAM records on the device costs (zsw_sam_batch, include/zoe_sw.h): n synthetic 150-base reads on the device against
a 2 kb reference, names r<i>, constant qualities, zsw_align_3pass_batch_from, then the SAM call over its records — the sizing call
alone, the full call, and the full call with ZSW_SAM_OMIT_SEQ and no qualities — everything device-resident, through the bare C ABI.
Per figure: the median of the timed steps and their min..max spread (host clocks around a call that ends in a device synchronise,
as tools/bench_annotate.py). Taken in the same run: a device-to-device hipMemcpy of as many bytes as the text has and the text's
copy to pinned host memory. From the shapes: the bytes a call has to read and write per read, and that traffic over the time as a
share of the rate the device-to-device copy reached (which reads and writes its bytes: 2 x bytes / time).
Before anything is timed the result is checked: on the device that the line offsets increase and end at *out_n_bytes, on the host
that a sample of lines is what Python formats from the same records.

    python tools/bench_sam.py [--reads 10000000] [--steps 7] [--warmup 2] [--out profiles/sam_bench.json]
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

import numpy as np
import torch

L, REF_LEN = 150, 2000
RNAME = b"ref"


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
    assert torch.cuda.is_available(), "bench_sam.py needs a GPU"
    import zoe_amd
    from zoe_amd import _lib, synth

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
    # names r<i>, built on the host once; constant qualities
    digits = np.char.add("r", np.arange(n).astype(str)).astype("S")
    name_len = np.char.str_len(digits).astype(np.int64)
    noff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(name_len, out=noff[1:])
    names = torch.from_numpy(np.frombuffer(b"".join(digits.tolist()), dtype=np.uint8).copy()).to(dev)
    d_noff = torch.from_numpy(noff).to(dev)
    quals = torch.full((n * L,), ord("I"), dtype=torch.uint8, device=dev)
    f_full, f_bare = _lib.ZswSamFields(), _lib.ZswSamFields()
    for f in (f_full, f_bare):
        f.qnames, f.qname_offsets, f.rname, f.rname_len, f.mapq = names.data_ptr(), d_noff.data_ptr(), RNAME, len(RNAME), 255
    f_full.quals = quals.data_ptr()
    n_bytes, n_bad = C.c_uint64(0), C.c_uint64(0)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def sam(f, flags, text, cap_bytes, off=None):
        return lib.zsw_sam_batch(h, C.byref(b), C.byref(f), flags, aln.data_ptr(), status.data_ptr(), inc.data_ptr(), op.data_ptr(), t_in,
                                 text.data_ptr() if text is not None else None, cap_bytes, C.byref(n_bytes), off.data_ptr() if off is not None else None,
                                 C.byref(n_bad), None)

    ctx.check(sam(f_full, 0, None, 0), profile_errors=False)
    full_bytes = int(n_bytes.value)
    text = torch.empty(full_bytes, dtype=torch.uint8, device=dev)
    ctx.check(sam(f_full, 0, text, full_bytes, offsets), profile_errors=False)
    torch.cuda.synchronize()
    assert int(n_bad.value) == 0
    # the self-check: offsets on the device, a sample of lines on the host
    assert int(offsets[0]) == 0 and int(offsets[n]) == full_bytes and bool((offsets[1:] > offsets[:-1]).all()), "line offsets do not increase to the total"
    sample = np.unique(np.concatenate([np.arange(min(n, 64)), np.linspace(0, n - 1, min(n, 2000)).astype(np.int64), np.arange(max(0, n - 64), n)]))
    idx = torch.from_numpy(sample).to(dev)
    h_aln = aln.view(n, 10)[idx].cpu().numpy().astype(np.uint32)
    h_status = status[idx].cpu().numpy()
    h_off = torch.stack([offsets[idx], offsets[idx + 1]], 1).cpu().numpy()
    h_reads = rb.bases.view(n, L)[idx].cpu().numpy()
    for k, i in enumerate(sample):
        r = h_aln[k]
        coff, cn = int(r[8]) | (int(r[9]) << 32), int(r[7])
        ci, co = inc[coff:coff + cn].cpu().numpy().astype(np.uint32), op[coff:coff + cn].cpu().numpy()
        seq = h_reads[k].tobytes().decode()
        if h_status[k] == 0:
            cigar = "".join(f"{int(a)}{chr(int(o))}" for a, o in zip(ci, co)) or "*"
            want = f"r{i}\t0\tref\t{int(r[1]) + 1}\t255\t{cigar}\t*\t0\t0\t{seq}\t{'I' * L}\tAS:i:{int(r[0])}\n"
        else:
            want = f"r{i}\t4\t*\t0\t0\t*\t*\t0\t0\t{seq}\t{'I' * L}\n"
        got = text[int(h_off[k, 0]):int(h_off[k, 1])].cpu().numpy().tobytes().decode()
        assert got == want, (i, got, want)
    ctx.check(sam(f_bare, _lib.SAM_OMIT_SEQ, None, 0), profile_errors=False)
    bare_bytes = int(n_bytes.value)
    n_some = int((status == 0).sum())

    r_align = timed(align, args.steps, args.warmup)
    r_sizing = timed(lambda: sam(f_full, 0, None, 0), args.steps, args.warmup)
    r_full = timed(lambda: sam(f_full, 0, text, full_bytes), args.steps, args.warmup)
    r_bare = timed(lambda: sam(f_bare, _lib.SAM_OMIT_SEQ, text, full_bytes), args.steps, args.warmup)
    copy_dst = torch.empty(full_bytes, dtype=torch.uint8, device=dev)
    r_copy = timed(lambda: copy_dst.copy_(text), args.steps, args.warmup)  # hipMemcpy device to device of *out_n_bytes bytes
    del copy_dst
    pinned = torch.empty(full_bytes, dtype=torch.uint8, pin_memory=True)
    r_d2h = timed(lambda: pinned.copy_(text, non_blocking=True), args.steps, args.warmup)
    copy_rate = 2 * full_bytes / (1e-3 * r_copy["median_ms"])  # bytes read + written per second
    # Bytes a call has to move, from the shapes. The length launch reads a record (40), a status (1), two name offsets (16; every
    # offset is read as the end of one line and the start of the next, counted once: 8) and the read's ciglets (5 each), and writes a
    # length (8) and a shape (1); the scan reads the lengths and writes the starts (16); the write launch reads record, status, name
    # offsets, shape and the line's start again (40 + 1 + 8 + 1 + 8), the ciglets of a mapped read, the name, the bases and the
    # qualities, and writes the text.
    name_bytes = int(noff[n])
    sizing = n * (40 + 1 + 8 + 8 + 1) + 5 * t_in + n * 16
    write_fixed = n * (40 + 1 + 8 + 1 + 8) + 5 * t_in + name_bytes
    full_traffic = sizing + write_fixed + 2 * n * L + full_bytes
    bare_traffic = sizing + write_fixed + bare_bytes
    for r, nbytes in ((r_sizing, sizing), (r_full, full_traffic), (r_bare, bare_traffic)):
        r["bytes_per_read"] = nbytes / n
        r["bytes"] = nbytes
        r["share_of_copy_rate"] = nbytes / (1e-3 * r["median_ms"]) / copy_rate
        r["share_of_align_call"] = r["median_ms"] / r_align["median_ms"]
    result = {"reads": n, "read_len": L, "ref_len": REF_LEN, "steps": args.steps, "warmup": args.warmup,
              "timing": "host clock around a call that ends in a device synchronise; median and min..max of the timed steps",
              "reads_with_alignment": n_some, "ciglets": t_in, "text_bytes": full_bytes, "text_bytes_per_read": full_bytes / n,
              "text_bytes_omit_seq_no_quals": bare_bytes, "record_bytes": n * 41 + 5 * t_in,
              "device_copy_rate_bytes_per_s": copy_rate, "zsw_align_3pass_batch_from": r_align, "sam_sizing_call": r_sizing, "sam_full_call": r_full,
              "sam_full_call_omit_seq_no_quals": r_bare, "device_to_device_copy_of_the_text": r_copy, "device_to_pinned_host_copy_of_the_text": r_d2h}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
