"""What parsing FASTA on the device costs (zsw_fasta_parse_batch, include/zoe_sw.h), and whether it costs the same per byte whatever
the records look like — the claim its sequence pass over tiles of the text is built for. The same n synthetic 150-base reads
(zsw_synth_reads_host) with fixed-width names as
  (a) n records, each sequence on one line,
  (b) n records wrapped at 60 columns,
  (c) ONE record of the same bases wrapped at 60 columns,
uploaded once and parsed through the bare C ABI with the capacities that always suffice (no sizing call); and as yardsticks in the
same run (d) zsw_fastq_parse_batch over the same reads as FASTQ and a device-to-device copy of each text's size (torch's copy_ of a
contiguous uint8 tensor: one hipMemcpyAsync). Per call: the median of the timed steps and their min..max (host clocks around a call
that ends in a device synchronise, as tools/bench_pileup.py). Before anything is timed the parser's arrays are compared with the
arrays the text was built from.

Not measured: host-staged calls, chunked use (ZSW_FASTA_FINAL unset, ZSW_FASTA_CONTINUED), hardware counters.

    python tools/bench_fasta.py [--reads 10000000] [--steps 7] [--warmup 2] [--out profiles/fasta_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

import bench_fastq as bq

L, NAME_W, WIDTH = bq.L, bq.NAME_W, 60


def single_line_text(reads, names):
    n = reads.shape[0]
    t = np.empty((n, 1 + NAME_W + 1 + L + 1), dtype=np.uint8)
    t[:, 0] = ord(">")
    t[:, 1:1 + NAME_W] = names
    t[:, 1 + NAME_W] = 10
    t[:, 2 + NAME_W:2 + NAME_W + L] = reads
    t[:, -1] = 10
    return t


def wrapped_text(reads, names):
    n = reads.shape[0]
    pieces = [(k, min(k + WIDTH, L)) for k in range(0, L, WIDTH)]
    t = np.empty((n, 1 + NAME_W + 1 + L + len(pieces)), dtype=np.uint8)
    t[:, 0] = ord(">")
    t[:, 1:1 + NAME_W] = names
    t[:, 1 + NAME_W] = 10
    p = 2 + NAME_W
    for lo, hi in pieces:
        t[:, p:p + hi - lo] = reads[:, lo:hi]
        t[:, p + hi - lo] = 10
        p += hi - lo + 1
    return t


def one_record_text(reads):
    flat = reads.reshape(-1)
    rows = len(flat) // WIDTH
    body = np.empty((rows, WIDTH + 1), dtype=np.uint8)
    body[:, :WIDTH] = flat[:rows * WIDTH].reshape(rows, WIDTH)
    body[:, WIDTH] = 10
    tail = np.concatenate([flat[rows * WIDTH:], [10]]).astype(np.uint8) if len(flat) > rows * WIDTH else np.empty(0, dtype=np.uint8)
    return np.concatenate([np.frombuffer(b">one_record the whole set\n", dtype=np.uint8), body.reshape(-1), tail])


class Parsed:
    def __init__(self, ctx, text_host):
        self.ctx = ctx
        dev = torch.device("cuda", 0)
        self.text = torch.from_numpy(text_host.reshape(-1)).to(dev)
        n = self.n_bytes = self.text.numel()
        self.base_cap, self.name_cap, self.record_cap = n, n, n // 4 + 1
        self.bases = torch.empty(self.base_cap, dtype=torch.uint8, device=dev)
        self.names = torch.empty(self.name_cap, dtype=torch.uint8, device=dev)
        self.off = torch.empty(self.record_cap + 1, dtype=torch.int64, device=dev)
        self.noff = torch.empty(self.record_cap + 1, dtype=torch.int64, device=dev)
        self.info = (C.c_uint64 * 9)()

    def parse(self):
        ctx = self.ctx
        ctx.check(ctx.lib.zsw_fasta_parse_batch(ctx.h, self.text.data_ptr(), self.n_bytes, 1, 1, self.bases.data_ptr(), self.base_cap, self.off.data_ptr(),
                                                self.names.data_ptr(), self.name_cap, self.noff.data_ptr(), self.record_cap, self.info, None), profile_errors=False)

    def verify(self, flat, off, names):
        dev = self.text.device
        info = [int(x) for x in self.info]
        n = len(off) - 1
        assert info[0] == n and info[1] == len(flat) and info[2] == len(names) and info[3] == self.n_bytes and info[4] == 0, info
        assert torch.equal(self.bases[:len(flat)], torch.from_numpy(flat).to(dev)), "bases"
        assert torch.equal(self.names[:len(names)], torch.from_numpy(names).to(dev)), "names"
        assert torch.equal(self.off[:n + 1], torch.from_numpy(off.astype(np.int64)).to(dev)), "offsets"
        return info


def cell(ctx, text_host, flat, off, names, args):
    p = Parsed(ctx, text_host)
    p.parse()
    torch.cuda.synchronize()
    info = p.verify(flat, off, names)
    out = {"records": info[0], "n_bytes": p.n_bytes, "bases": info[1], "name_bytes": info[2], "min_len": info[7], "max_len": info[8]}
    out["fasta_parse"] = bq.timed(p.parse, args.steps, args.warmup)
    dst = torch.empty_like(p.text)
    out["copy_device_to_device"] = bq.timed(lambda: dst.copy_(p.text), args.steps, args.warmup)
    del dst
    fp = out["fasta_parse"]
    fp["ratio_to_copy"] = fp["median_ms"] / out["copy_device_to_device"]["median_ms"]
    fp["text_bytes_per_s"] = p.n_bytes / (1e-3 * fp["median_ms"])
    fp["ns_per_byte"] = 1e6 * fp["median_ms"] / p.n_bytes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fasta.py needs a GPU"
    import zoe_amd
    from zoe_amd import synth

    n = args.reads
    ctx = zoe_amd.SwContext.get(0)
    ref = synth.reference_host(2000)
    result = {"read_len": L, "name_bytes_per_read": NAME_W, "wrap": WIDTH, "steps": args.steps, "warmup": args.warmup,
              "timing": "host clock around a call that ends in a device synchronise; median and min..max of the timed steps",
              "not_measured": ["host-staged calls", "chunked use (ZSW_FASTA_FINAL unset, ZSW_FASTA_CONTINUED)", "hardware counters"]}
    reads = synth.reads_host(ref, 0, n, L)
    names = bq.names_of(n)
    flat, off = reads.reshape(-1), np.arange(n + 1, dtype=np.int64) * L
    result["a_single_line_records"] = cell(ctx, single_line_text(reads, names), flat, off, names.reshape(-1), args)
    torch.cuda.empty_cache()
    result["b_wrapped_records"] = cell(ctx, wrapped_text(reads, names), flat, off, names.reshape(-1), args)
    torch.cuda.empty_cache()
    result["c_one_wrapped_record"] = cell(ctx, one_record_text(reads), flat, np.array([0, len(flat)], dtype=np.int64), np.frombuffer(b"one_record the whole set", dtype=np.uint8),
                                          args)
    torch.cuda.empty_cache()
    text, fq_names, quals = bq.fixed_text(reads)  # (d) the same reads as FASTQ
    p = bq.Parsed(ctx, text)
    p.parse()
    torch.cuda.synchronize()
    p.verify(flat, off, fq_names, quals)
    d = {"n_bytes": p.n_bytes, "fastq_parse": bq.timed(p.parse, args.steps, args.warmup)}
    dst = torch.empty_like(p.text)
    d["copy_device_to_device"] = bq.timed(lambda: dst.copy_(p.text), args.steps, args.warmup)
    d["fastq_parse"]["text_bytes_per_s"] = p.n_bytes / (1e-3 * d["fastq_parse"]["median_ms"])
    d["fastq_parse"]["ns_per_byte"] = 1e6 * d["fastq_parse"]["median_ms"] / p.n_bytes
    result["d_fastq_same_reads"] = d
    a, c = result["a_single_line_records"]["fasta_parse"], result["c_one_wrapped_record"]["fasta_parse"]
    result["per_byte_ratio_c_to_a"] = c["ns_per_byte"] / a["ns_per_byte"]
    result["per_byte_ratio_b_to_a"] = result["b_wrapped_records"]["fasta_parse"]["ns_per_byte"] / a["ns_per_byte"]
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
