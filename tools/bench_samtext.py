"""What parsing SAM on the device costs (zsw_sam_parse_batch, include/zoe_sw.h): n synthetic 150-base reads on the device against a
2 kb reference, names r<i>, constant qualities, zsw_align_3pass_batch_from and zsw_sam_batch give the text (device-resident, as
tools/bench_sam.py builds it); then the parse over that text through the bare C ABI with ZSW_SAMTEXT_FINAL | ZSW_SAMTEXT_QUAL_FORWARD,
RNAME and ref_len given, into arrays of exactly the sizes the sizing call reports — the sizing call alone, the full call, and the
full call without the optional outputs (quals, names, strand, parsed). Timed in the same run, as yardsticks: zsw_sam_batch writing
the text from the same records, and a device-to-device copy of the text (torch's copy_ of a contiguous uint8 tensor: one
hipMemcpyAsync), the floor for a call that must read the text. Per figure: the median of the timed steps and their min..max (host clocks around a call that ends
in a device synchronise, as tools/bench_sam.py). Before anything is timed the parsed records, ciglets, bases and names are compared on
the device with the arrays the text was written from.

Not measured: host-staged calls, chunked use (ZSW_SAMTEXT_FINAL unset), texts with long CIGARs or many optional fields, per-kernel times.

    python tools/bench_samtext.py [--reads 10000000] [--steps 7] [--warmup 2] [--out profiles/samtext_bench.json]
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
    assert torch.cuda.is_available(), "bench_samtext.py needs a GPU"
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
        rc = lib.zsw_align_3pass_batch_from(h, C.byref(b), 8, 256, 0, aln.data_ptr(), status.data_ptr(), tier.data_ptr(), inc.data_ptr(), op.data_ptr(), cap,
                                            C.byref(total), None)
        if rc == -1 and total.value > cap:
            cap = int(total.value)
            continue
        ctx.check(rc)
        break
    t_in = int(total.value)
    digits = np.char.add("r", np.arange(n).astype(str)).astype("S")
    noff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.char.str_len(digits).astype(np.int64), out=noff[1:])
    names = torch.from_numpy(np.frombuffer(b"".join(digits.tolist()), dtype=np.uint8).copy()).to(dev)
    d_noff = torch.from_numpy(noff).to(dev)
    quals = torch.full((n * L,), ord("I"), dtype=torch.uint8, device=dev)
    f = _lib.ZswSamFields()
    f.qnames, f.qname_offsets, f.quals, f.rname, f.rname_len, f.mapq = names.data_ptr(), d_noff.data_ptr(), quals.data_ptr(), RNAME, len(RNAME), 255
    n_bytes, n_bad = C.c_uint64(0), C.c_uint64(0)

    def sam(text, cap_bytes):
        return lib.zsw_sam_batch(h, C.byref(b), C.byref(f), 0, aln.data_ptr(), status.data_ptr(), inc.data_ptr(), op.data_ptr(), t_in,
                                 text.data_ptr() if text is not None else None, cap_bytes, C.byref(n_bytes), None, C.byref(n_bad), None)

    ctx.check(sam(None, 0), profile_errors=False)
    text_bytes = int(n_bytes.value)
    text = torch.empty(text_bytes, dtype=torch.uint8, device=dev)
    ctx.check(sam(text, text_bytes), profile_errors=False)
    torch.cuda.synchronize()
    assert int(n_bad.value) == 0

    info = (C.c_uint64 * _lib.SAMTEXT_INFO_WORDS)()
    flags = _lib.SAMTEXT_FINAL | _lib.SAMTEXT_QUAL_FORWARD

    def parse(o):
        return lib.zsw_sam_parse_batch(h, text.data_ptr(), text_bytes, _lib.MEM_DEVICE, flags, RNAME, len(RNAME), REF_LEN, C.byref(o), info, None)

    sizing = _lib.ZswSamParseOut()
    ctx.check(parse(sizing), profile_errors=False)
    rep = [int(x) for x in info]
    n_rec, n_bases, n_names, n_cig = rep[_lib.SAMTEXT_INFO_RECORDS], rep[_lib.SAMTEXT_INFO_BASES], rep[_lib.SAMTEXT_INFO_NAME_BYTES], rep[_lib.SAMTEXT_INFO_CIGLETS]
    assert rep[_lib.SAMTEXT_INFO_ERROR] == 0 and n_rec == n and n_bases == n * L and n_names == int(noff[n])
    out = {"bases": torch.empty(n_bases, dtype=torch.uint8, device=dev), "quals": torch.empty(n_bases, dtype=torch.uint8, device=dev),
           "offsets": torch.empty(n_rec + 1, dtype=torch.int64, device=dev), "qnames": torch.empty(n_names, dtype=torch.uint8, device=dev),
           "qname_offsets": torch.empty(n_rec + 1, dtype=torch.int64, device=dev), "aln": torch.empty(n_rec * 10, dtype=torch.int32, device=dev),
           "status": torch.empty(n_rec, dtype=torch.uint8, device=dev), "inc": torch.empty(max(n_cig, 1), dtype=torch.int32, device=dev),
           "op": torch.empty(max(n_cig, 1), dtype=torch.uint8, device=dev), "strand": torch.empty(n_rec, dtype=torch.uint8, device=dev),
           "parsed": torch.empty(n_rec * 24, dtype=torch.uint8, device=dev)}
    full, bare = _lib.ZswSamParseOut(), _lib.ZswSamParseOut()
    for o in (full, bare):
        o.base_cap, o.name_cap, o.ciglet_cap, o.record_cap = n_bases, n_names, n_cig, n_rec
    for k, v in out.items():
        setattr(full, k, v.data_ptr())
        if k not in ("quals", "qnames", "qname_offsets", "strand", "parsed"):
            setattr(bare, k, v.data_ptr())
    ctx.check(parse(full), profile_errors=False)
    torch.cuda.synchronize()
    # the self-check, on the device: what was parsed is what the text was written from
    some = status == 0
    a_in, a_out = aln.view(n, 10), out["aln"].view(n, 10)
    assert bool((out["status"] == torch.where(some, 0, 2).to(torch.uint8)).all()), "status"
    assert bool((a_out[some][:, :8] == a_in[some][:, :8]).all()) and not bool(a_out[~some].any()), "records"
    assert n_cig == int(a_in[some][:, 7].sum()) and rep[_lib.SAMTEXT_INFO_MAPPED] == int(some.sum())
    assert bool((out["bases"] == rb.bases).all()) and bool((out["quals"] == quals).all()) and bool((out["qnames"] == names).all()) and bool((out["qname_offsets"] == d_noff).all())
    first = (a_in[:, 8].to(torch.int64) | (a_in[:, 9].to(torch.int64) << 32))[some][:2000]
    got_first = (a_out[:, 8].to(torch.int64) | (a_out[:, 9].to(torch.int64) << 32))[some][:2000]
    cnt = a_in[some][:2000, 7].cpu().numpy()
    h_inc, h_op, g_inc, g_op = inc.cpu().numpy(), op.cpu().numpy(), out["inc"].cpu().numpy(), out["op"].cpu().numpy()
    for s0, s1, c in zip(first.cpu().numpy(), got_first.cpu().numpy(), cnt):
        assert np.array_equal(h_inc[s0:s0 + c], g_inc[s1:s1 + c]) and np.array_equal(h_op[s0:s0 + c], g_op[s1:s1 + c]), "ciglets"
    del h_inc, h_op, g_inc, g_op

    r_sizing = timed(lambda: parse(sizing), args.steps, args.warmup)
    r_full = timed(lambda: parse(full), args.steps, args.warmup)
    r_bare = timed(lambda: parse(bare), args.steps, args.warmup)
    r_sam = timed(lambda: sam(text, text_bytes), args.steps, args.warmup)
    copy_dst = torch.empty(text_bytes, dtype=torch.uint8, device=dev)
    r_copy = timed(lambda: copy_dst.copy_(text), args.steps, args.warmup)
    del copy_dst
    copy_rate = 2 * text_bytes / (1e-3 * r_copy["median_ms"])
    # bytes a full call has to move at least: the text once per pass that reads it (newline count, newline positions, line pass; the
    # gather reads SEQ, QUAL, QNAME and the CIGAR again), and the outputs
    outputs = 2 * n_bases + n_names + 16 * (n_rec + 1) + n_rec * (40 + 1 + 1 + 24) + 5 * n_cig
    floor = 3 * text_bytes + 2 * n_bases + n_names + outputs
    for r in (r_sizing, r_full, r_bare):
        r["share_of_sam_batch"] = r["median_ms"] / r_sam["median_ms"]
        r["ns_per_record"] = 1e6 * r["median_ms"] / n
    r_full["least_bytes"] = floor
    r_full["share_of_copy_rate"] = floor / (1e-3 * r_full["median_ms"]) / copy_rate
    result = {"reads": n, "read_len": L, "ref_len": REF_LEN, "steps": args.steps, "warmup": args.warmup,
              "timing": "host clock around a call that ends in a device synchronise; median and min..max of the timed steps",
              "text_bytes": text_bytes, "text_bytes_per_read": text_bytes / n, "records": n_rec, "mapped": rep[_lib.SAMTEXT_INFO_MAPPED], "ciglets": n_cig,
              "device_copy_rate_bytes_per_s": copy_rate, "parse_sizing_call": r_sizing, "parse_full_call": r_full, "parse_without_optional_outputs": r_bare,
              "zsw_sam_batch_writing_the_text": r_sam, "device_to_device_copy_of_the_text": r_copy}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
