#!/usr/bin/env python3
"""Headline benchmark: batched striped Smith-Waterman, many 150 bp reads vs one 2 kb reference, score-only.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One process per GPU.  A "step" is one pass of the hot path (`read.into_local_profile(..).sw_score_from_i8(reference)`
for every read, i.e. zsw_score_batch_from) over the rank's batch of synthetic reads, already resident in HBM,
followed — for N > 1 — by the RCCL all-gather of the per-read scores and statuses (the only exchange the path
has; one collective per step, zoe_amd/dist.py).  `value` is the library's default path: the seeded exact pass
(zsw_score_seed.hip, zsw_score_band.hip: k-mer anchors, a band of diagonals around them, bound checks, the full pass for the
reads handed back —
bit-identical to computing every cell, which the run verifies on ALL reads and reports beside it).
Workloads (BASELINE.json):
  N = 1  configs[1]: 10 M reads on the GPU.
  N > 1  configs[3]: 500 M reads in total, sharded by contiguous index ranges [i*n/N, (i+1)*n/N) (62.5 M per GPU at
         N = 8); the counter-based generator lets every rank synthesise exactly its own shard on its own GPU.
--reads-per-gpu overrides both with a fixed per-GPU batch (weak scaling).

Prints ONE JSON line (rank 0).  `roofline` is measured live with HIP events on the kernel's stream.
A plain run sets up, warms up, times the steps and prints the line.  --full adds, after the timed region: the oracle check
of a slice of the batch (--verify), the headline workload with every cell computed and compared (`full_pass_every_cell`), the
other configs (`secondary`), `cpu_baseline` (the restated Zoe CPU path, oracle/, AVX2 w256, on the host cores over a bounded
sample) and, for N > 1, the gather-order checks.
--dump-outputs DIR writes what the last timed step returned (rank 0's batch; a fixed sample of 2^21 reads of a larger one) as
DIR/score.npy, status.npy, tier.npy (float64 / float32) and read_index.npy (the reads sampled, float64).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

READ_LEN = 150
REF_LEN = 2000
ALGO_BYTES_PER_READ = READ_LEN + 4  # read bytes in + u32 score out
# Per-read instruction counts and HBM counters of the kernels below are CONSTANTS from committed rocprofv3 --pmc passes (separate
# runs; the gfx950 x2 correction for wide streaming reads is NOT applied to FETCH_SIZE: the loads are 8-byte strip-boundary rows and
# 4-byte code words, the raw counter is reported), not measurements of this run — the bench line says so. They live in
# profiles/constants.json together with the sha256 of the .hip_fatbin section of the library they were measured on
# (tools/refresh_constants.py); a bench run on a library with another hash marks every figure derived from them "stale".
CONSTANTS_FILE = "profiles/constants.json"


def load_constants():
    with open(os.path.join(ROOT, CONSTANTS_FILE)) as f:
        return json.load(f)


PC = load_constants()
PMC_PROFILE = PC["band"]["source"]
WINDOW_HBM_BYTES_PER_READ = PC["band"]["hbm_bytes_per_read"]   # FETCH_SIZE + WRITE_SIZE per read of the batch, both launches of the banded kernel (tier 1 seed_band_kernel<16,4,0>, tier 2 <48,2,0>)
WINDOW_VALU_PER_READ = PC["band"]["valu_per_read"]            # SQ_INSTS_VALU per read of the batch, both launches
VALU_PEAK_SOURCE = "profiles/r01_valu_issue_rates_ubench.txt"  # this repo's micro-benchmark (tools/ubench.hip), not a figure of the guide
TOTAL_READS_MULTI_GPU = 500_000_000  # BASELINE.json configs[3]
HBM_PEAK_GBS = 8000.0               # MI355X_MICROARCH.md: 8 TB/s spec
# v_pk_{add,sub,max}_i16 and v_perm_b32 issue at one wave64 instruction per 4 cycles per SIMD on gfx950
# (profiles/r01_valu_issue_rates_ubench.txt: half the v_fma_f32/v_add_u32 rate), i.e. 16 lanes/clk/SIMD.
VALU_LANE_OPS_PEAK = 256 * 4 * 16 * 2.4e9  # 256 CU x 4 SIMD x 16 lanes/clk x 2.4 GHz (32-bit lane-ops/s)
PACKED_OPS_PER_CELL_PAIR = 7.5      # zsw_score.hip score_kernel_v2 inner loop: 7.5 packed VALU per two cells
DUMP_SAMPLE = 1 << 21               # reads dumped by --dump-outputs: 2^21 x (8 + 4 + 4 + 8) B = 48 MiB at most


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true", help="after the timed region, also run the checks and other measurements "
                    "(oracle check, full pass, secondary configs, CPU baseline; each can be left out with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's results as DIR/<name>.npy")
    ap.add_argument("--reads-per-gpu", type=int, default=0, help="fixed batch per GPU (weak scaling); default: 10 M at N = 1, "
                    "500 M / N at N > 1 (BASELINE.json configs[1] / configs[3])")
    ap.add_argument("--total-reads", type=int, default=TOTAL_READS_MULTI_GPU, help="total reads of the N > 1 workload")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target wall time of the CPU baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--verify", type=int, default=2048, help="reads checked against the oracle after the timed region")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short config-3 / config-5 measurements")
    ap.add_argument("--no-full-pass", action="store_true", help="skip the run of the headline workload with every cell computed (and the comparison of all results)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to rehearse the "
                    "multi-rank path on a one-GPU box together with --single-device)")
    ap.add_argument("--single-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def dump_outputs(result, n_reads: int, out_dir: str):
    """The score batch of the last timed step as .npy files: every read of a batch of up to DUMP_SAMPLE reads, else the same
    seeded sample of DUMP_SAMPLE read indices in every run (the inputs are seeded too, so two builds compare read by read)."""
    import torch

    if n_reads <= DUMP_SAMPLE:
        idx = np.arange(n_reads, dtype=np.int64)
    else:
        idx = np.sort(np.random.default_rng(20240917).choice(n_reads, DUMP_SAMPLE, replace=False))
    sel = torch.from_numpy(idx).to(result.score.device)
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"score": result.score[sel].cpu().numpy().view(np.uint32).astype(np.float64),
              "status": result.status[sel].cpu().numpy().astype(np.float32),
              "tier": result.tier[sel].cpu().numpy().astype(np.float32),
              "read_index": idx.astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def host_cores() -> int:
    """Usable host cores: affinity mask capped by the cgroup CPU quota (a 1-GPU box gets a share of the host)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]))))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, q // int(f.read())))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(reference: bytes, target_s: float):
    """Restated Zoe CPU path (oracle/zoe_cpu_fast.cpp): fresh i8x32 -> i16x16 profiles per read, all host cores."""
    from oracle import oracle
    from zoe_amd import synth

    oracle.build()
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    cores = host_cores()
    probe = synth.reads_host(reference, 0, 1000 * cores, READ_LEN)
    t0 = time.perf_counter()
    oracle.batch_score_w256(8, sc, probe, reference, fixed_len=READ_LEN, threads=cores)
    probe_rate = probe.shape[0] / (time.perf_counter() - t0)
    n = int(max(probe.shape[0], min(probe_rate * target_s, 8_000_000)))
    reads = synth.reads_host(reference, 0, n, READ_LEN)
    t0 = time.perf_counter()
    oracle.batch_score_w256(8, sc, reads, reference, fixed_len=READ_LEN, threads=cores)
    dt = time.perf_counter() - t0
    # short side samples: one thread, i16-direct, and one shared reference-side profile
    def rate(fn, k):
        t = time.perf_counter()
        fn(reads[:k])
        return k / (time.perf_counter() - t)

    k1 = max(2000, min(n, int(rate_guess_1t(rate, cores) * 3)))
    variants = {
        "from_i8_fresh_profile_1_thread": rate(lambda r: oracle.batch_score_w256(8, sc, r, reference, fixed_len=READ_LEN, threads=1), k1),
        "from_i16_fresh_profile_all_threads": rate(
            lambda r: oracle.batch_score_w256(16, sc, r, reference, fixed_len=READ_LEN, threads=cores), min(n, int(probe_rate * 3))),
        "from_i8_shared_reference_profile_all_threads": rate(
            lambda r: oracle.batch_score_shared_w256(8, sc, r, reference, fixed_len=READ_LEN, threads=cores), min(n, int(probe_rate * 3))),
    }
    return {
        "value": n / dt,
        "unit": "read-alignments/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{n} of the same synthetic 150 bp reads vs the 2 kb reference, sw_score_from_i8 (i8x32 -> i16x16, "
                  f"fresh profile per read), restated Zoe CPU path (AVX2), {cores} threads, {dt:.1f} s",
        "variants_reads_per_s": variants,
    }


def rate_guess_1t(rate_fn, cores):
    """Reads/s of one thread, estimated on a tiny probe so the 1-thread sample lasts about 3 s."""
    from oracle import oracle
    from zoe_amd import synth

    ref = synth.reference_host(REF_LEN)
    probe = synth.reads_host(ref, 0, 1000, READ_LEN)
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    t = time.perf_counter()
    oracle.batch_score_w256(8, sc, probe, ref, fixed_len=READ_LEN, threads=1)
    return 1000 / (time.perf_counter() - t)


def file_tag(rel: str) -> str:
    """name + first 12 hex digits of the sha256 of a committed profile file (so a constant can be traced to its source)."""
    import hashlib

    try:
        with open(os.path.join(ROOT, rel), "rb") as f:
            return f"{rel}#sha256:{hashlib.sha256(f.read()).hexdigest()[:12]}"
    except OSError:
        return rel + " (missing)"


WAVE_INSTR_PEAK = 256 * 4 * 2.4e9 / 4  # wave64 VALU instructions/s: 1,024 SIMDs, one per 4 cycles at 2.4 GHz (VALU_PEAK_SOURCE)
# VALU wave-instructions per read of the pass-2 / score kernels, from committed rocprofv3 --pmc SQ_INSTS_VALU passes
# (constants from those profiles, not measured in the bench run): tools/pmc_entry.py, one entry point per run, every kernel of
# the call summed (profiles/r03_secondary_valu.txt; per-phase budget of the packed alignment kernel: profiles/r02_align_pk_pmc.txt)
SECONDARY_VALU_PROFILE = PC["secondary"]["source"]
ALIGN_PK_VALU_PER_READ = PC["secondary"]["align_pass2_valu_per_read"]   # align_kernel_pk<16,10> + <32,5> (pass 2 alone: what pass2_kernel_ms times)
ALIGN_PK_PROFILE = SECONDARY_VALU_PROFILE
RANGES_VALU_PER_READ = PC["secondary"]["ranges_valu_per_read"]          # banded kernel (MODE 2) + reverse pass + handed-back reads + seed kernel
THREEPASS_VALU_PER_READ = PC["secondary"]["threepass_valu_per_read"]    # the same + threepass_kernel
# FETCH_SIZE + WRITE_SIZE per read of the same calls (separate --pmc passes, raw counters), same file
RANGES_HBM_PER_READ = PC["secondary"]["ranges_hbm_per_read"]
THREEPASS_HBM_PER_READ = PC["secondary"]["threepass_hbm_per_read"]
MIXED_HBM_PER_READ = PC["secondary"]["mixed_hbm_per_read"]
ALIGN_HBM_PER_READ = PC["secondary"]["align_hbm_per_read"]              # the flag ring of pass 2 (30 kB per read) and its read-back by the traceback
PROTEIN_PROFILE = PC["protein"]["source"]
PROTEIN_VALU_PER_READ = PC["protein"]["valu_per_read"]   # prune_strip_kernel<24,WIDE> + prune_window_kernel<24,4,32,0,WIDE> + score_kernel_v2<..,WIDE> over the reads handed back
PROTEIN_HBM_PER_READ = PC["protein"]["hbm_per_read"]     # the strip's boundary stream written, read back by the window kernel
MIXED_VALU_PER_READ = PC["secondary"]["mixed_valu_per_read"]            # 75-400 bp vs 30 kb


def library_hash():
    from zoe_amd import build

    try:
        return build.fatbin_sha256()
    except (OSError, RuntimeError):
        return None


LIB_HASH = library_hash()


def constants_state(section: str):
    """where a constant comes from and whether it was measured on the library this run loads"""
    src = PC[section]
    return {"source": file_tag(src["source"]), "measured_on_fatbin_sha256": src.get("fatbin_sha256"), "running_fatbin_sha256": LIB_HASH,
            "stale": src.get("fatbin_sha256") != LIB_HASH}


def _stale_of(source):
    """True if the profile file `source` was taken from another library build than the one loaded (profiles/constants.json)"""
    for sec in PC.values():
        if isinstance(sec, dict) and sec.get("source") == source:
            return sec.get("fatbin_sha256") != LIB_HASH
    return True


def rooflines(algo_bytes: float, kernel_s: float, valu_instr: float = None, source: str = None, traffic_bytes: float = None):
    """The two roofs of a secondary entry: algorithmic bytes over the kernels' time against HBM (`traffic`: the FETCH_SIZE +
    WRITE_SIZE counters of a committed PMC pass of the same call, over the same time), and (where a committed PMC pass gives
    the instruction count) issued VALU wave-instructions against the 4-cycle issue rate."""
    out = {"roofline": {"bound": "hbm", "achieved": algo_bytes / kernel_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": algo_bytes / kernel_s / 1e9 / HBM_PEAK_GBS,
                        "traffic": traffic_bytes / kernel_s / 1e9 if traffic_bytes else None,
                        "traffic_bytes_per_launch": traffic_bytes, "traffic_measured_in_this_run": False if traffic_bytes else None,
                        "traffic_source": file_tag(source) if (traffic_bytes and source) else None,
                        "traffic_stale": _stale_of(source) if (traffic_bytes and source) else None,
                        "algorithmic_bytes_per_launch": algo_bytes, "kernel_ms": kernel_s * 1e3}}
    if valu_instr:
        out["valu_roofline"] = {"bound": "valu", "achieved": valu_instr / kernel_s / 1e9, "peak": WAVE_INSTR_PEAK / 1e9,
                                "unit": "G wave64 VALU instructions/s", "frac": valu_instr / kernel_s / WAVE_INSTR_PEAK,
                                "instruction_count_source": file_tag(source) if source else None,
                                "instruction_count_measured_in_this_run": False, "stale": _stale_of(source), "valu_peak_source": VALU_PEAK_SOURCE}
    return out


def full_pass_headline(zoe_amd, ctx, profiles, reference, default, n_reads, steps):
    """The headline workload again with every cell computed (zsw_set_option(ZSW_OPTION_EXACT_PRUNING, 0): score_kernel_v2 over
    the whole batch, the path `value` measured in rounds 1-2). Every score, status and tier of the default path (`default`)
    must equal it, all n_reads of them."""
    import torch

    from zoe_amd import _lib

    ctx.set_option(_lib.OPTION_EXACT_PRUNING, 0)
    try:
        got = profiles.sw_score_from_i8(reference)
        torch.cuda.synchronize()
        ctx.timing_enable(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            got = profiles.sw_score_from_i8(reference)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ks, launches = ctx.timing_read()
        ctx.timing_enable(False)
    finally:
        ctx.set_option(_lib.OPTION_EXACT_PRUNING, 1)
    same = bool(torch.equal(got.score, default.score) and torch.equal(got.status, default.status) and torch.equal(got.tier, default.tier))
    if not same:
        raise SystemExit("PARITY FAILURE: the default (seeded) pass differs from the full pass")
    per_launch = ks / max(launches, 1)
    cells = n_reads * READ_LEN * REF_LEN
    return {
        "reads_per_s": n_reads * steps / dt,
        "kernel": "zsw::score_kernel_v2<4,38,0>",
        "kernel_ms": per_launch * 1e3,
        "default_path_identical": f"all {n_reads} scores, statuses and tiers compared in this run",
        "valu_roofline_frac": cells / per_launch / 2 * PACKED_OPS_PER_CELL_PAIR / VALU_LANE_OPS_PEAK if per_launch > 0 else None,
    }


def secondary_configs(zoe_amd, synth, ctx, matrix):
    """Measurements of the other BASELINE.json configs on this GPU (after the timed region; not part of `value`):
    configs[2] full traceback at its full size (10 M reads) and configs[4] mixed lengths vs a 30 kb reference (1 M reads),
    plus the neighbouring entry points on 1 M reads. Every entry carries its own roofline(s)."""
    import torch

    out = {}
    ref2k = synth.reference_host(REF_LEN)

    def timed(fn):
        """result, wall seconds and kernel seconds of the faster of two calls after a warm-up call (a single call now and then
        catches an allocation of the caching allocators: 3-pass 1 M reads measured 61 and 36 ms in consecutive bench runs)"""
        fn()  # warm-up (allocations, first-launch costs)
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            ctx.timing_read()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ks, _ = ctx.timing_read()
            if best is None or dt < best[1]:
                best = (r, dt, ks)
            del r
        return best

    def with_full_first_pass(fn):
        """the same call with every cell of the first pass computed (ZSW_OPTION_EXACT_PRUNING 0): must be bit-identical"""
        from zoe_amd import _lib

        ctx.set_option(_lib.OPTION_EXACT_PRUNING, 0)
        try:
            return timed(fn)
        finally:
            ctx.set_option(_lib.OPTION_EXACT_PRUNING, 1)

    ctx.timing_enable(True)
    # configs[2]: 10 M reads, sw_simd_align with CIGAR, bit-exact vs the CPU path of the same <T, N>
    n_full = 10_000_000
    rb = synth.reads_device(ctx, ref2k, 0, n_full, READ_LEN)
    prof = zoe_amd.into_local_profile(rb, matrix, -10, -1, device=ctx.device)
    a, dt, ks = timed(lambda: prof.sw_align_from_i8(zoe_amd.SeqSrc.Reference(ref2k)))
    n_cig = int(len(a.inc))
    n_some = int((a.status == 0).sum())
    entry = {"reads_per_s_end_to_end_incl_d2h": n_full / dt, "pass2_kernel_ms": ks * 1e3, "pass2_kernel_ms_per_1M_reads": ks * 1e3 / (n_full / 1e6),
             "ciglets": n_cig, "aligned_reads": n_some,
             "call": "into_local_profile(..).sw_align_from_i8(SeqSrc::Reference(ref)) (CIGAR of the i16x16 / i8x32 tier), 10 M reads (BASELINE.json configs[2] at full size)",
             "kernel": "zsw::align_kernel_pk<16,10> (+ <32,5> for the reads that answer at i8x32); pass 1 = the seeded exact pass (seed_band_kernel<16,4,3> forward + reversed: is there exactly one optimal alignment? DESIGN.md §4.2)"}
    # algorithmic bytes: read in, record out (score, 4 coordinates, 2 lengths, count, offset = 40 B), 5 B per ciglet
    entry.update(rooflines(n_full * (READ_LEN + 4.0) + n_some * 40.0 + n_cig * 5.0, ks, ALIGN_PK_VALU_PER_READ * n_full, ALIGN_PK_PROFILE,
                           ALIGN_HBM_PER_READ * n_full))
    ap, dtp, ksp = with_full_first_pass(lambda: prof.sw_align_from_i8(zoe_amd.SeqSrc.Reference(ref2k)))
    entry["with_full_first_pass"] = {"reads_per_s_end_to_end_incl_d2h": n_full / dtp, "pass2_kernel_ms": ksp * 1e3,
                                       "identical": bool(np.array_equal(ap.status, a.status) and np.array_equal(ap.records, a.records)
                                                         and np.array_equal(ap.inc, a.inc) and np.array_equal(ap.op, a.op))}
    del ap
    out["align_full_traceback_10M_x_150bp_vs_2kb"] = entry
    del a, prof, rb
    torch.cuda.empty_cache()

    rb = synth.reads_device(ctx, ref2k, 0, 1_000_000, READ_LEN)
    prof = zoe_amd.into_local_profile(rb, matrix, -10, -1, device=ctx.device)
    a3, dt, ks = timed(lambda: prof.sw_align_from_i8_3pass(zoe_amd.SeqSrc.Reference(ref2k)))
    entry = {"reads_per_s_end_to_end_incl_d2h": 1_000_000 / dt, "kernels_ms": ks * 1e3, "ciglets": int(len(a3.inc)),
             "call": "into_local_profile(..).sw_align_from_i8_3pass(SeqSrc::Reference(ref)) (three_pass.rs: ranges, then no-gaps / banded / scalar in the box)"}
    entry.update(rooflines(1e6 * (READ_LEN + 4.0) + float((a3.status == 0).sum()) * 40.0 + len(a3.inc) * 5.0, ks, THREEPASS_VALU_PER_READ * 1e6,
                           SECONDARY_VALU_PROFILE, THREEPASS_HBM_PER_READ * 1e6))
    ap, dtp, ksp = with_full_first_pass(lambda: prof.sw_align_from_i8_3pass(zoe_amd.SeqSrc.Reference(ref2k)))
    entry["with_full_first_pass"] = {"reads_per_s_end_to_end_incl_d2h": 1_000_000 / dtp, "kernels_ms": ksp * 1e3,
                                       "identical": bool(np.array_equal(ap.status, a3.status) and np.array_equal(ap.records, a3.records)
                                                         and np.array_equal(ap.inc, a3.inc) and np.array_equal(ap.op, a3.op))}
    out["align_3pass_1M_x_150bp_vs_2kb"] = entry
    del a3, ap
    # score + ranges (striped.rs:355-388) and the sneaky_snake filter on the window each read maps to
    sp = zoe_amd.StripedProfileBatch(rb, matrix, -10, -1, T="i16", N=16, device=ctx.device)
    rg, dt, ks = timed(lambda: sp.sw_score_ranges(zoe_amd.SeqSrc.Reference(ref2k)))
    entry = {"reads_per_s": 1_000_000 / dt, "kernels_ms": ks * 1e3, "call": "StripedProfile::<i16,16,5>::sw_score_ranges(SeqSrc::Reference(ref))"}
    entry.update(rooflines(1e6 * (READ_LEN + 4.0 + 16.0), max(ks, 1e-9) if ks > 0 else dt, RANGES_VALU_PER_READ * 1e6, SECONDARY_VALU_PROFILE, RANGES_HBM_PER_READ * 1e6))
    rp_, dtp, ksp = with_full_first_pass(lambda: sp.sw_score_ranges(zoe_amd.SeqSrc.Reference(ref2k)))
    entry["with_full_first_pass"] = {"reads_per_s": 1_000_000 / dtp, "kernels_ms": ksp * 1e3,
                                       "identical": all(bool(torch.equal(getattr(rp_, f), getattr(rg, f)))
                                                        for f in ("score", "status", "ref_start", "ref_end", "query_start", "query_end"))}
    del rp_
    out["score_ranges_1M_x_150bp_vs_2kb"] = entry
    st = (rg.ref_start.to(torch.int64) - rg.query_start.to(torch.int64)).clamp(0, REF_LEN - READ_LEN).to(torch.int32)
    ln = torch.full_like(st, READ_LEN)
    flt, dt, ks = timed(lambda: zoe_amd.sneaky_snake(ref2k, rb, st, ln, 0.05))
    entry = {"pairs_per_s": 1_000_000 / dt, "pass_fraction": float((flt == 1).float().mean()),
             "call": "sneaky_snake(&ref[start..start+150], read, 0.05) per read"}
    entry.update(rooflines(1e6 * (2 * READ_LEN + 8.0 + 1.0), dt))
    out["sneaky_snake_1M_x_150bp_windows"] = entry
    del rg, flt, sp, rb, prof
    torch.cuda.empty_cache()
    # configs[4]: mixed lengths vs a 30 kb reference, bucketed by strip configuration on the device
    ref30k = synth.reference_host(30000)
    rr = synth.reads_ragged_device(ctx, ref30k, 0, 1_000_000, 75, 400)
    pm = zoe_amd.into_local_profile(rr, matrix, -10, -1, device=ctx.device)
    _, dt, ks = timed(lambda: pm.sw_score_from_i8(ref30k))
    ctx.timing_enable(False)
    total_bases = float(rr.offsets[-1])
    cells = total_bases * 30000
    entry = {"reads_per_s": 1_000_000 / dt, "kernel_ms": ks * 1e3,
             "call": "sw_score_from_i8, reads bucketed by strip configuration on the device, seeded exact pass per length class"}
    entry.update(rooflines(total_bases + 1e6 * (8.0 + 4.0), dt, MIXED_VALU_PER_READ * 1e6, SECONDARY_VALU_PROFILE, MIXED_HBM_PER_READ * 1e6))
    entry["gcups"] = "equivalent: the cells of the full matrices per second (the seeded pass computes about one in ninety of them)"
    entry["gcups_equivalent"] = cells / dt / 1e9
    del entry["gcups"]
    ctx.timing_enable(True)
    seeded_mixed = pm.sw_score_from_i8(ref30k)
    handed_back = ctx.prune_rescored()
    got, dtp, ksp = with_full_first_pass(lambda: pm.sw_score_from_i8(ref30k))
    ctx.timing_enable(False)
    lane_ops = cells / dtp / 2 * PACKED_OPS_PER_CELL_PAIR
    entry["handed_back_fraction"] = handed_back / 1_000_000
    entry["with_full_first_pass"] = {"reads_per_s": 1_000_000 / dtp, "gcups": cells / dtp / 1e9, "kernels_ms": ksp * 1e3,
                                     "valu_roofline_frac_useful_cells": lane_ops / VALU_LANE_OPS_PEAK,
                                     "identical": bool(torch.equal(got.score, seeded_mixed.score) and torch.equal(got.status, seeded_mixed.status)
                                                       and torch.equal(got.tier, seeded_mixed.tier))}
    out["score_mixed_1M_x_75_400bp_vs_30kb"] = entry
    del rr, pm, got, seeded_mixed
    torch.cuda.empty_cache()
    out["score_divergence_sweep"] = divergence_sweep(ctx)
    out.update(protein_and_shared(zoe_amd, synth, ctx, matrix, timed, with_full_first_pass))
    return out


def divergence_sweep(ctx):
    """The default score path against read divergence (tools/bench_divergence.py): 1 M reads of 150 bases per rate — pieces of the
    2 kb reference with x % substitutions, x / 10 % single-base indels and 2 % unrelated reads; every result compared with the full pass."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_divergence

    rows = bench_divergence.sweep(ctx, 1_000_000, [1, 2, 3, 5, 8, 12])
    if not all(r["identical"] for r in rows):
        raise SystemExit("PARITY FAILURE: the default (seeded) pass differs from the full pass on diverged reads")
    return {"reads": 1_000_000, "read_len": READ_LEN, "ref_len": REF_LEN, "rows": rows,
            "note": "handed_back_fraction includes the 2 % unrelated reads of every set; a 1 M-read batch runs at about 0.6 of the 10 M-read batch's rate"}


def protein_and_shared(zoe_amd, synth, ctx, matrix, timed, with_full_first_pass):
    """Two more users of the score pass on 1 M reads each: a 25-letter alphabet (the reference's amino-acid matrices are
    WeightMatrix<i8, 25>, src/data/matrices/aa.rs; default first pass: the column-pruned one) and the shared-profile
    role (one profile from the 2 kb reference, the reads as the other sequence: sw/mod.rs:63-67, profile_set.rs:552-560; 4.5)."""
    import torch

    out = {}
    n = 1_000_000
    keys = b"ACDEFGHIKLMNPQRSTVWYBJZX*"
    rng = np.random.default_rng(3)
    w = rng.integers(-4, 3, size=(25, 25))
    w = np.minimum(w, w.T)
    np.fill_diagonal(w, rng.integers(4, 12, size=25))
    pm = zoe_amd.WeightMatrix.new_custom(zoe_amd.ByteIndexMap.new(keys, b"X"), w.astype(np.int8))
    alpha = np.frombuffer(keys[:20], dtype=np.uint8)
    refa = rng.choice(alpha, 2000).astype(np.uint8)
    start = rng.integers(0, 2000 - READ_LEN, size=n)
    reads = refa[start[:, None] + np.arange(READ_LEN)[None, :]]
    reads = np.where(rng.random((n, READ_LEN)) < 0.03, rng.choice(alpha, (n, READ_LEN)), reads).astype(np.uint8)
    junk = rng.random(n) < 0.02
    reads[junk] = rng.choice(alpha, (int(junk.sum()), READ_LEN))
    rb = zoe_amd.ReadBatch.from_fixed(torch.from_numpy(reads.reshape(-1)).to(f"cuda:{ctx.device}"), READ_LEN)
    prof = zoe_amd.into_local_profile(rb, pm, -11, -1, device=ctx.device)
    ctx.timing_enable(True)
    got, dt, ks = timed(lambda: prof.sw_score_from_i8(refa.tobytes()))
    handed_back = ctx.prune_rescored()
    entry = {"reads_per_s": n / dt, "kernels_ms": ks * 1e3, "handed_back_fraction": handed_back / n,
             "call": "sw_score_from_i8, 25-letter BLOSUM-shaped matrix, 150 residues vs 2,000 (pieces of the reference, 3 % substituted, + 2 % unrelated)",
             "kernel": "prune_strip_kernel<24,WIDE> + prune_window_kernel<24,4,32,0,WIDE>, score_kernel_v2<..,WIDE> over the reads handed back"}
    entry.update(rooflines(n * (READ_LEN + 4.0), ks if ks > 0 else dt, PROTEIN_VALU_PER_READ * n, PROTEIN_PROFILE, PROTEIN_HBM_PER_READ * n))
    full, dtp, ksp = with_full_first_pass(lambda: prof.sw_score_from_i8(refa.tobytes()))
    entry["with_full_first_pass"] = {"reads_per_s": n / dtp, "kernels_ms": ksp * 1e3,
                                       "identical": bool(torch.equal(full.score, got.score) and torch.equal(full.status, got.status) and torch.equal(full.tier, got.tier))}
    out["score_protein_25_letters_1M_x_150_vs_2000"] = entry
    del rb, prof, got, full
    torch.cuda.empty_cache()
    # the shared-profile role on the headline's reads
    ref2k = synth.reference_host(REF_LEN)
    rb = synth.reads_device(ctx, ref2k, 0, n, READ_LEN)
    sp = zoe_amd.SharedStripedProfile(ref2k, matrix, -10, -1, "i16", 16, device=ctx.device)
    sc_, dt_s, ks_s = timed(lambda: sp.sw_score(rb))
    en, dt_e, ks_e = timed(lambda: sp.sw_score_ends(zoe_amd.SeqBatchSrc.Reference(rb)))
    en0, dt_e0, _ = with_full_first_pass(lambda: sp.sw_score_ends(zoe_amd.SeqBatchSrc.Reference(rb)))
    rg, dt_r, ks_r = timed(lambda: sp.sw_score_ranges(zoe_amd.SeqBatchSrc.Reference(rb)))
    rg0, dt_r0, _ = with_full_first_pass(lambda: sp.sw_score_ranges(zoe_amd.SeqBatchSrc.Reference(rb)))
    # its alignments: 3-pass on all the reads, layout-exact (sw_simd_align's own traceback) on the first 100,000
    a3, dt_a3, _ = timed(lambda: sp.sw_align_3pass(zoe_amd.SeqBatchSrc.Query(rb)))
    n_ex = min(n, 100_000)
    rb_ex = zoe_amd.ReadBatch.from_fixed(rb.bases[: n_ex * READ_LEN], READ_LEN)
    ax, dt_ax, _ = timed(lambda: sp.sw_align(zoe_amd.SeqBatchSrc.Query(rb_ex)))
    ctx.timing_enable(False)
    out["shared_profile_1M_x_150bp_vs_2kb"] = {
        "align_3pass_reads_per_s_end_to_end_incl_d2h": n / dt_a3,
        "align_exact_100k_reads_per_s_end_to_end_incl_d2h": n_ex / dt_ax,
        "align_note": "sw_align_3pass / sw_align(SeqSrc::Query(read)) with the shared profile; exact: reads with exactly one optimal alignment (gapless or one gap run) come from the certificate pass, the rest from the literal striped recurrence over the shared sequence's profile (align_shared_kernel_h)",
        "score_reads_per_s": n / dt_s, "score_ends_reads_per_s": n / dt_e, "score_ends_kernels_ms": ks_e * 1e3,
        "score_ranges_reads_per_s": n / dt_r, "score_ranges_kernels_ms": ks_r * 1e3,
        "score_ranges_every_read_by_the_exact_shared_kernels": {
            "reads_per_s": n / dt_r0, "identical": all(bool(torch.equal(getattr(rg0, f), getattr(rg, f)))
                                                        for f in ("score", "status", "ref_start", "ref_end", "query_start", "query_end"))},
        "call": "StripedProfile::<i16,16,5>::new(reference) reused for every read: sw_score(read) / sw_score_ends / sw_score_ranges(SeqSrc::Reference(read))",
        "kernel": "the seeded pass with the roles swapped (seed_band_kernel<16|32,.,3>: ends + 'the maximum sits in one cell'; ranges: again over the reversed sequences), shared_ends_kernel for every other read",
        "every_read_by_the_exact_shared_kernel": {"score_ends_reads_per_s": n / dt_e0,
                                                    "identical": all(bool(torch.equal(getattr(en0, f), getattr(en, f))) for f in ("score", "status", "ref_end", "query_end"))}}
    return out


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N > 1")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no GPU visible (there is no CPU fallback path)")
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)

    import zoe_amd
    from zoe_amd import synth
    from zoe_amd.dist import GatheredResults, ResultSlab, gather_slabs, shard_capacity, shard_range, slab_bytes

    ctx = zoe_amd.SwContext.get(local_rank)
    reference = synth.reference_host(REF_LEN)
    matrix = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")  # the reference's test/bench constants (sw/mod.rs:465-471)
    if args.reads_per_gpu > 0:  # fixed batch per GPU
        n_total, scaling = args.reads_per_gpu * world, "weak"
        workload = f"{args.reads_per_gpu} synthetic {READ_LEN} bp reads per GPU"
    elif world == 1:  # BASELINE.json configs[1]
        n_total, scaling = 10_000_000, "weak"
        workload = f"BASELINE.json configs[1]: {n_total} synthetic {READ_LEN} bp reads on one GPU"
    else:  # BASELINE.json configs[3]
        n_total, scaling = args.total_reads, "strong"
        workload = (f"BASELINE.json configs[3]: {n_total} synthetic {READ_LEN} bp reads in total, sharded over {world} GPUs "
                    f"({shard_capacity(n_total, world)} per GPU), per-read best-score gather over RCCL")
    workload += f" vs one {REF_LEN} bp reference, score-only (sw_score_from_i8, w256 preset; 2/-5/N ignored, gaps -10/-1)"
    first, n_local = shard_range(n_total, rank, world)
    reads = synth.reads_device(ctx, reference, first, n_local, READ_LEN)
    profiles = zoe_amd.LocalProfilesBatch.new_with_w256(reads, matrix, -10, -1, device=local_rank)
    dev = torch.device("cuda", local_rank)

    # N > 1: the kernel writes scores + statuses into a byte slab, and ONE all-gather per step moves the slabs (zoe_amd/dist.py).
    # Two slabs alternate: the gather of step k runs (asynchronously, on RCCL's stream, ordered after the producing kernel)
    # under the kernel of step k+1, which fills the other slab; only the next gather, or the closing fence, waits for it.
    gather_on_host = world > 1 and args.backend != "nccl"  # gloo rehearsal of the same code path on a one-GPU box
    if world > 1:
        cap = shard_capacity(n_total, world)
        counts = [shard_range(n_total, r, world)[1] for r in range(world)]
        slabs = [ResultSlab(cap, device=dev), ResultSlab(cap, device=dev)]
        host_slabs = [ResultSlab(cap), ResultSlab(cap)] if gather_on_host else None
        gathered = GatheredResults(world, cap, counts, device=None if gather_on_host else dev)
    pending = []
    step_no = [0]

    def drain():
        for work in pending:
            work.wait()
        pending.clear()

    def step():
        if world == 1:
            return profiles.sw_score_from_i8(reference)
        k = step_no[0] % 2
        step_no[0] += 1
        r = profiles.sw_score_from_i8(reference, out=slabs[k])
        src = slabs[k]
        if gather_on_host:
            host_slabs[k].buf.copy_(slabs[k].buf)  # rehearsal only: gloo gathers host memory
            src = host_slabs[k]
        drain()  # the gather of the previous step had this step's kernel launch to hide behind
        pending.append(gather_slabs(src, gathered, async_op=True))
        return r

    def fence():
        if world > 1:
            drain()
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    fence()
    ctx.timing_enable(True)
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = step()
    fence()
    dt = time.perf_counter() - t0
    kern_s, launches = ctx.timing_read()
    win_s, win_launches = ctx.timing_read_window()
    ctx.timing_enable(False)
    handed_back = ctx.prune_rescored()
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if gather_on_host else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if world > 1 and args.full:
        # the gathered array must be every rank's shard in read order: own shard, and the first read of every other shard
        # against a single-process score of the same (regenerated) read
        mine = gathered.score_of_rank(rank)
        assert torch.equal(mine.cpu(), last.score.cpu()), "all-gather order"
        if rank == 0:
            probe = zoe_amd.LocalProfilesBatch.new_with_w256(_first_reads(zoe_amd, synth, ctx, reference, n_total, world), matrix, -10, -1,
                                                             device=local_rank).sw_score_from_i8(reference)
            got = torch.stack([gathered.score_of_rank(r)[0] for r in range(world)]).cpu()
            assert torch.equal(got, probe.score.cpu()), "gathered shards do not start with the right reads"
    if rank == 0 and args.dump_outputs:
        dump_outputs(last, n_local, args.dump_outputs)

    # parity spot check outside the timed region (rank 0): a slice of the batch against the oracle
    verified = None
    if rank == 0 and args.full and args.verify > 0:
        from oracle import oracle

        oracle.build()
        nv = min(args.verify, n_local)
        host = synth.reads_host(reference, first, nv, READ_LEN)
        sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
        ws, wst, _ = oracle.batch_score_w256(8, sc, host, reference, fixed_len=READ_LEN, threads=min(8, os.cpu_count() or 1))
        gs = last.score[:nv].cpu().numpy().view("uint32")
        gst = last.status[:nv].cpu().numpy()
        verified = bool((gs == ws).all() and (gst == wst).all())
        if not verified:
            raise SystemExit("PARITY FAILURE: GPU scores differ from the oracle")

    if rank == 0:
        total_reads = n_total * args.steps
        value = total_reads / dt
        pass_s = kern_s / max(launches, 1)             # the whole first pass: seed + sort + window + full pass over the handed-back reads
        seeded = win_launches > 0
        kern = win_s / win_launches if seeded else pass_s  # the dominant kernel alone
        kernel_name = "zsw::seed_band_kernel<16,4,0> over every read (16-column strips, band 8/6) + <48,2,0> over the reads that fail in it (48-column strips, band 25/12): two launches per step" if seeded else "zsw::score_kernel_v2<4,38,0>"
        achieved = ALGO_BYTES_PER_READ * n_local / kern / 1e9 if kern > 0 else 0.0
        traffic = WINDOW_HBM_BYTES_PER_READ * n_local if (seeded and WINDOW_HBM_BYTES_PER_READ) else None
        out = {
            "metric": "read-alignments/sec (150 bp vs 2 kb ref)",
            "value": value,
            "unit": "read-alignments/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": "int16",
            "data": "synthetic",
            "config": {
                "workload": workload,
                "total_reads": n_total,
                "reads_per_gpu": n_local,
                "read_len": READ_LEN,
                "ref_len": REF_LEN,
                "parallelism": (f"reads sharded over {world} GPU(s), contiguous index ranges; one RCCL all-gather per step of a "
                                f"{slab_bytes(shard_capacity(n_total, world))} B slab per rank (u32 scores + u8 statuses), issued under the next step's kernel"
                                if world > 1 else "single GPU"),
            },
            "path": {
                "default": "seeded exact pass (zsw_score_seed.hip, zsw_score_band.hip): k-mer anchors -> a band of diagonals around the anchor -> bound checks -> full pass for the reads handed back; "
                           "bit-identical to computing every cell" if seeded else "full pass (every cell)",
                "handed_back_fraction": handed_back / max(n_local, 1),
                "first_pass_ms": pass_s * 1e3,
                "gcups_equivalent": value * READ_LEN * REF_LEN / 1e9,
                "data_dependence": "`value` holds for reads within a few per cent of the reference (the synthetic set: 1 % substitutions, 2 % unrelated reads = "
                                   "the handed-back fraction). The proof rests on k-mers the read shares with the reference: beyond about one substitution per "
                                   "ten bases a read is scored over all its cells. Data-independent floor: full_pass_every_cell.reads_per_s; the curve between: "
                                   "secondary.score_divergence_sweep (both with --full)",
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic / kern / 1e9 if (traffic and kern > 0) else None,
                "traffic_bytes_per_launch": traffic,
                "traffic_measured_in_this_run": False,
                "traffic_stale": constants_state("band")["stale"] if traffic else None,
                "traffic_source": ("constant from rocprofv3 --pmc FETCH_SIZE, WRITE_SIZE passes of the same kernel and workload: " + file_tag(PMC_PROFILE))
                                  if traffic else None,
                "kernel": kernel_name,
                "kernel_ms": kern * 1e3,
                "kernel_ms_source": "HIP events recorded around the kernel launches (both tiers and the selection between them) on their stream, inside this run",
                "algorithmic_bytes_per_read": ALGO_BYTES_PER_READ,
                "note": "HBM is not the binding roof: packed-i16 VALU issue is (valu_roofline); the seeded pass raises the rate by computing fewer cells; traffic is the strip boundary of the banded kernel",
            },
            "parity_checked_reads": args.verify if verified else 0,
        }
        if seeded and WINDOW_VALU_PER_READ:
            instr = WINDOW_VALU_PER_READ * n_local
            out["valu_roofline"] = {"bound": "valu", "achieved": instr / kern / 1e9, "peak": WAVE_INSTR_PEAK / 1e9,
                                    "unit": "G wave64 VALU instructions/s", "frac": instr / kern / WAVE_INSTR_PEAK, "kernel": kernel_name,
                                    "instruction_count_source": file_tag(PMC_PROFILE), "instruction_count_measured_in_this_run": False,
                                    "library_fatbin_sha256": LIB_HASH, "stale": constants_state("band")["stale"],
                                    "valu_peak_source": "one wave64 packed/perm/max3 instruction per 4 cycles per SIMD: " + file_tag(VALU_PEAK_SOURCE)}
        if world == 1 and args.full and not args.no_full_pass:
            out["full_pass_every_cell"] = full_pass_headline(zoe_amd, ctx, profiles, reference, last, n_local, args.steps)
        if world == 1 and args.full and not args.no_secondary:
            del reads, profiles, last
            torch.cuda.empty_cache()
            out["secondary"] = secondary_configs(zoe_amd, synth, ctx, matrix)
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(reference, args.cpu_seconds)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _first_reads(zoe_amd, synth, ctx, reference, n_total, world):
    """The first read of every rank's shard as one small batch (for the gather-order check)."""
    import torch
    from zoe_amd.dist import shard_range

    parts = [synth.reads_device(ctx, reference, shard_range(n_total, r, world)[0], 1, READ_LEN).bases.view(-1) for r in range(world)]
    return zoe_amd.ReadBatch.from_fixed(torch.cat(parts), READ_LEN)


if __name__ == "__main__":
    main()
