"""What parsing FASTQ on the device costs (zsw_fastq_parse_batch, include/zoe_sw.h): the text of n synthetic 150-base reads with
fixed-width names, built on the host as a 2-D byte array from zsw_synth_reads_host's reads, uploaded once, and parsed through the bare
C ABI with the capacities that always suffice (no sizing call). Timed in the same run, as yardsticks: (b) a device-to-device copy of
n_bytes (torch's copy_ of a contiguous uint8 tensor: one hipMemcpyAsync), the floor for a call that must read the text and write
nearly as much; (c) zsw_sam_batch over the same reads with the names and qualities the parser wrote, which moves the same kind of
volume and formats decimals on top; (d) the getline loop of examples/zsw_driver.cpp on a 1 M-read file on the host. Also 1 M mixed
75..400-base reads. Per call: the median of the timed steps and their min..max (host clocks around a call that ends in a device
synchronise, as tools/bench_pileup.py). Before anything is timed the parser's arrays are compared with the arrays the text was built
from.

Not measured: host-staged calls, CRLF files, chunked use (ZSW_FASTQ_FINAL unset), per-kernel times.

    python tools/bench_fastq.py [--reads 10000000] [--steps 7] [--warmup 2] [--out profiles/fastq_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

L = 150
NAME_W = 10  # 'r' and nine digits

GETLINE_LOOP = r"""
// the FASTQ loop of examples/zsw_driver.cpp, alone
#include <chrono>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
int main(int argc, char** argv) {
    const auto t0 = std::chrono::steady_clock::now();
    std::ifstream fq(argv[1]);
    std::vector<std::string> names, reads, quals;
    std::string h, s, p, q;
    while (std::getline(fq, h) && std::getline(fq, s) && std::getline(fq, p) && std::getline(fq, q)) {
        if (h.empty() || h[0] != '@') return 1;
        names.push_back(h.substr(1, h.find_first_of(" \t") == std::string::npos ? std::string::npos : h.find_first_of(" \t") - 1));
        reads.push_back(s);
        quals.push_back(q);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::cout << reads.size() << ' ' << ms << '\n';
    return argc > 2 ? (int)names.size() : 0;
}
"""


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


def names_of(n):
    idx = np.arange(n, dtype=np.int64)
    out = np.empty((n, NAME_W), dtype=np.uint8)
    out[:, 0] = ord("r")
    for k in range(1, NAME_W):
        out[:, k] = 48 + (idx // 10 ** (NAME_W - 1 - k)) % 10
    return out


def quals_of(bases):
    return (40 + bases % 23).astype(np.uint8)  # '(' .. '>'


def fixed_text(reads):
    """(n, L) bases -> the FASTQ text as an (n, row) byte array, the names, the qualities"""
    n = reads.shape[0]
    names, quals = names_of(n), quals_of(reads)
    row = 1 + NAME_W + 1 + L + 1 + 2 + L + 1
    t = np.empty((n, row), dtype=np.uint8)
    t[:, 0] = ord("@")
    t[:, 1:1 + NAME_W] = names
    p = 1 + NAME_W
    t[:, p] = 10
    t[:, p + 1:p + 1 + L] = reads
    p += 1 + L
    t[:, p], t[:, p + 1], t[:, p + 2] = 10, ord("+"), 10
    t[:, p + 3:p + 3 + L] = quals
    t[:, p + 3 + L] = 10
    return t, names, quals


def ragged_text(flat, off):
    """ragged bases -> the FASTQ text (1-D), the names, the qualities"""
    n = len(off) - 1
    lens = np.diff(off).astype(np.int64)
    names, quals = names_of(n), quals_of(flat)
    rec = 1 + NAME_W + 1 + lens + 3 + lens + 1
    start = np.concatenate([[0], np.cumsum(rec)]).astype(np.int64)
    t = np.empty(int(start[-1]), dtype=np.uint8)
    s = start[:-1]
    t[s] = ord("@")
    for k in range(NAME_W):
        t[s + 1 + k] = names[:, k]
    seq0 = s + 2 + NAME_W
    t[seq0 - 1] = 10
    within = np.arange(len(flat), dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), lens)
    t[np.repeat(seq0, lens) + within] = flat
    t[seq0 + lens], t[seq0 + lens + 1], t[seq0 + lens + 2] = 10, ord("+"), 10
    t[np.repeat(seq0 + lens + 3, lens) + within] = quals
    t[seq0 + 2 * lens + 3] = 10
    return t, names, quals


class Parsed:
    def __init__(self, ctx, text_host):
        self.ctx = ctx
        dev = torch.device("cuda", 0)
        self.text = torch.from_numpy(text_host.reshape(-1)).to(dev)
        n = self.n_bytes = self.text.numel()
        self.base_cap, self.name_cap, self.record_cap = n // 2, n, n // 8 + 1
        self.bases = torch.empty(self.base_cap, dtype=torch.uint8, device=dev)
        self.quals = torch.empty(self.base_cap, dtype=torch.uint8, device=dev)
        self.names = torch.empty(self.name_cap, dtype=torch.uint8, device=dev)
        self.off = torch.empty(self.record_cap + 1, dtype=torch.int64, device=dev)
        self.noff = torch.empty(self.record_cap + 1, dtype=torch.int64, device=dev)
        self.info = (C.c_uint64 * 9)()

    def parse(self):
        ctx = self.ctx
        ctx.check(ctx.lib.zsw_fastq_parse_batch(ctx.h, self.text.data_ptr(), self.n_bytes, 1, 1, self.bases.data_ptr(), self.quals.data_ptr(), self.base_cap,
                                                self.off.data_ptr(), self.names.data_ptr(), self.name_cap, self.noff.data_ptr(), self.record_cap, self.info, None),
                  profile_errors=False)

    def verify(self, flat, off, names, quals):
        dev = self.text.device
        info = [int(x) for x in self.info]
        n = len(off) - 1
        assert info[0] == n and info[1] == len(flat) and info[2] == names.size and info[3] == self.n_bytes and info[4] == 0, info
        assert torch.equal(self.bases[:len(flat)], torch.from_numpy(flat).to(dev)), "bases"
        assert torch.equal(self.quals[:len(flat)], torch.from_numpy(quals.reshape(-1)).to(dev)), "qualities"
        assert torch.equal(self.names[:names.size], torch.from_numpy(names.reshape(-1)).to(dev)), "names"
        assert torch.equal(self.off[:n + 1], torch.from_numpy(off.astype(np.int64)).to(dev)), "offsets"
        assert torch.equal(self.noff[:n + 1], torch.arange(n + 1, dtype=torch.int64, device=dev) * NAME_W), "name offsets"
        return info


def cell(ctx, ref, text_host, flat, off, names, quals, args, with_sam):
    from zoe_amd import _lib

    p = Parsed(ctx, text_host)
    p.parse()
    torch.cuda.synchronize()
    info = p.verify(flat, off, names, quals)
    n = info[0]
    out = {"reads": n, "n_bytes": p.n_bytes, "bases": info[1], "name_bytes": info[2], "min_len": info[7], "max_len": info[8],
           "bytes_written": 2 * info[1] + info[2] + 16 * (n + 1)}
    out["fastq_parse"] = timed(p.parse, args.steps, args.warmup)
    dst = torch.empty_like(p.text)
    out["copy_device_to_device"] = timed(lambda: dst.copy_(p.text), args.steps, args.warmup)
    del dst
    out["fastq_parse"]["ratio_to_copy"] = out["fastq_parse"]["median_ms"] / out["copy_device_to_device"]["median_ms"]
    out["fastq_parse"]["text_bytes_per_s"] = p.n_bytes / (1e-3 * out["fastq_parse"]["median_ms"])
    if with_sam:
        lib, h, dev = ctx.lib, ctx.h, p.text.device
        ctx.set_reference(ref)
        b = _lib.ZswBatch()
        b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem, b.encoding = p.bases.data_ptr(), p.off.data_ptr(), 0, n, 1, 0
        aln = torch.zeros(n * 10, dtype=torch.int32, device=dev)
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
        f = _lib.ZswSamFields()
        f.qnames, f.qname_offsets, f.quals = p.names.data_ptr(), p.noff.data_ptr(), p.quals.data_ptr()
        f.rname, f.rname_len, f.mapq = b"synthref", 8, 255
        n_out, n_bad = C.c_uint64(0), C.c_uint64(0)
        args_ = (h, C.byref(b), C.byref(f), 0, aln.data_ptr(), status.data_ptr(), inc.data_ptr(), op.data_ptr(), int(total.value))
        ctx.check(lib.zsw_sam_batch(*args_, None, 0, C.byref(n_out), None, C.byref(n_bad), None), profile_errors=False)
        text = torch.empty(int(n_out.value), dtype=torch.uint8, device=dev)
        sam = lambda: ctx.check(lib.zsw_sam_batch(*args_, text.data_ptr(), text.numel(), C.byref(n_out), None, C.byref(n_bad), None), profile_errors=False)
        out["sam_batch"] = timed(sam, args.steps, args.warmup)
        out["sam_batch"]["text_bytes"] = text.numel()
        fp, sb = out["fastq_parse"], out["sam_batch"]
        out["fastq_parse"]["ratio_to_sam_batch"] = fp["median_ms"] / sb["median_ms"]
        # the acceptance: not longer than zsw_sam_batch beyond the spread of the two
        out["parse_not_slower_than_sam_batch"] = bool(fp["median_ms"] <= sb["median_ms"] + (fp["max_ms"] - fp["min_ms"]) + (sb["max_ms"] - sb["min_ms"]))
    return out


def host_getline(text_host, n_reads, steps, warmup):
    """the driver's loop on the first n_reads records of the fixed-width text, compiled alone, timed like the calls -> ms"""
    with tempfile.TemporaryDirectory(prefix="zsw_fastq_bench_") as tmp:
        src, exe, fq = os.path.join(tmp, "loop.cpp"), os.path.join(tmp, "loop"), os.path.join(tmp, "reads.fq")
        open(src, "w").write(GETLINE_LOOP)
        subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], check=True)
        text_host[:n_reads].tofile(fq)
        times = []
        for step in range(warmup + steps):
            got, ms = subprocess.run([exe, fq], capture_output=True, text=True, check=True).stdout.split()
            assert int(got) == n_reads
            if step >= warmup:
                times.append(float(ms) * 1e-3)
        return dict(summary(times), reads=n_reads, file_bytes=int(text_host[:n_reads].size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fastq.py needs a GPU"
    import zoe_amd
    from zoe_amd import synth

    n = args.reads
    ctx = zoe_amd.SwContext.get(0)
    ctx.set_scoring(zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N"), -10, -1)
    ref = synth.reference_host(2000)
    result = {"read_len": L, "name_bytes_per_read": NAME_W, "steps": args.steps, "warmup": args.warmup,
              "timing": "host clock around a call that ends in a device synchronise; median and min..max of the timed steps",
              "not_measured": ["host-staged calls", "CRLF files", "chunked use (ZSW_FASTQ_FINAL unset)", "per-kernel times"]}
    reads = synth.reads_host(ref, 0, n, L)
    text, names, quals = fixed_text(reads)
    result["host_getline_loop"] = host_getline(text, min(n, 1_000_000), args.steps, args.warmup)
    result["fixed_150"] = cell(ctx, ref, text, reads.reshape(-1), np.arange(n + 1, dtype=np.int64) * L, names, quals, args, True)
    del text, reads, quals
    torch.cuda.empty_cache()
    m = min(n, 1_000_000)
    flat, off = synth.reads_ragged_host(ref, 5, m, 75, 400)
    flat = np.ascontiguousarray(flat[:int(off[-1])])
    text, names, quals = ragged_text(flat, off)
    result["mixed_75_400"] = cell(ctx, ref, text, flat, off, names, quals, args, False)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
