"""ZSW_OPTION_MIN_SCORE through the front ends: examples/zsw_driver --min-score T (reads below T become unmapped SAM records, every
other line stays byte for byte) and the Python wrapper (SwContext.set_min_score, the BELOW_MIN_SCORE status, the counters)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_driver_min_score_writes_reads_below_it_as_unmapped(tmp_path):
    """The FASTQ of tests/test_gpu_driver.py (200 synthetic 100-base reads, one of them all N). T = the median AS of the run without
    the flag: with --3pass --min-score T the reads of a smaller AS (and the unmapped one) are flag-4 records as the all-N read
    is today, the other lines are identical; with --score-only they print `*`. Without --3pass or --score-only the flag is refused."""
    from zoe_amd import build, synth

    exe = build.build_driver()
    ref = synth.reference_host(1200)
    reads = synth.reads_host(ref, 4242, 200, 100)
    reads[3] = ord("N")
    (tmp_path / "ref.fa").write_bytes(b">synthref test\n" + ref[:600] + b"\n" + ref[600:] + b"\n")
    with open(tmp_path / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d extra\n" % i + r.tobytes() + b"\n+\n" + b"I" * len(r) + b"\n")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(__import__("torch").__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")

    def drive(*flags):
        return subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), *flags], capture_output=True, text=True, env=env, timeout=300)

    plain = drive("--3pass")
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.splitlines()
    recs = [l for l in lines if not l.startswith("@")]
    assert len(recs) == 200
    score = np.array([int(l.split("\t")[11][5:]) if l.split("\t")[1] == "0" else 0 for l in recs])
    assert score[3] == 0 and (score > 0).sum() == 199
    T = int(np.median(score[score > 0]))
    below = score < T
    assert 20 <= below.sum() <= 180, (T, int(below.sum()))
    out = drive("--3pass", "--min-score", str(T))
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    k = 0
    for a, b in zip(lines, got):
        if a.startswith("@"):
            assert a == b
            continue
        if below[k]:
            f, g = a.split("\t"), b.split("\t")
            assert g == [f[0], "4", "*", "0", "0", "*", "*", "0", "0", f[9], f[10]], (k, b)
        else:
            assert a == b, k
        k += 1
    assert got[[i for i, l in enumerate(lines) if not l.startswith("@")][3]] == recs[3]  # the all-N read: unmapped either way, the same record
    plain_s, out_s = drive("--score-only"), drive("--score-only", "--min-score", str(T))
    assert plain_s.returncode == 0 and out_s.returncode == 0, plain_s.stderr + out_s.stderr
    for k, (a, b) in enumerate(zip(plain_s.stdout.splitlines(), out_s.stdout.splitlines())):
        assert b == (a.split("\t")[0] + "\t*" if below[k] else a), k
    refused = drive("--min-score", str(T))
    assert refused.returncode == 2 and "--3pass" in refused.stderr


def test_python_wrapper_round_trip(oracle):
    """SwContext.set_min_score / min_score_counts and the BELOW_MIN_SCORE status through LocalProfilesBatch: 2,048 synthetic reads,
    a quarter of them replaced by random bases, T = 225; the uncovered sw_align_from_i8 raises while T > 0."""
    import torch

    import zoe_amd
    from zoe_amd import _lib, synth

    assert zoe_amd.BELOW_MIN_SCORE == 4 and _lib.OPTION_MIN_SCORE == 2
    ctx = zoe_amd.SwContext.get(0)
    ref = synth.reference_host(2000)
    n, T = 2048, 225
    host = synth.reads_host(ref, 77, n, 150).copy()
    host[::4] = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, (n // 4, 150))]
    rb = zoe_amd.ReadBatch.from_fixed(torch.from_numpy(host.reshape(-1)).cuda(), 150)
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    ws, wst, wt = oracle.batch_score_w256(8, sc, host, ref, fixed_len=150, threads=8)
    below = (wst == 2) | ((wst == 0) & (ws < T))
    assert n // 4 <= below.sum() < n
    prof = zoe_amd.LocalProfilesBatch.new_with_w256(rb, dna, -10, -1)
    ctx.set_min_score(T)
    try:
        got = prof.sw_score_from_i8(ref)
        cnt = ctx.min_score_counts()
        aln = prof.sw_align_from_i8_3pass(zoe_amd.SeqSrc.Reference(ref))
        with pytest.raises(_lib.ZswError) as e:
            prof.sw_align_from_i8(zoe_amd.SeqSrc.Reference(ref))
        assert e.value.code == -4 and "ZSW_OPTION_MIN_SCORE" in str(e.value)
        with pytest.raises(_lib.ZswError):
            ctx.set_min_score(-1)
    finally:
        ctx.set_min_score(0)
    status = got.status.cpu().numpy()
    assert np.array_equal(status, np.where(below, zoe_amd.BELOW_MIN_SCORE, wst))
    assert np.array_equal(got.score.cpu().numpy(), np.where(below, 0, ws)) and np.array_equal(got.tier.cpu().numpy(), np.where(below, 0, wt))
    i_below, i_some = int(np.nonzero(below)[0][0]), int(np.nonzero(~below)[0][0])
    assert got.maybe_aligned(i_below) == ("BelowMinScore", None) and got.maybe_aligned(i_some) == ("Some", int(ws[i_some]))
    assert cnt[3] == int(below.sum()) == cnt[0] + cnt[1] + cnt[2] and cnt[0] >= 400  # most of the 512 random reads by the whole-read bound at least
    assert np.array_equal(aln.status, np.where(below, zoe_amd.BELOW_MIN_SCORE, wst))
    assert aln.key(i_below) == (4, 0, (0, 0), (0, 0), "", 0, 0) and int(aln.records[i_below]["n_ciglets"]) == 0
    assert aln.key(i_some)[1] == int(ws[i_some])
    assert ctx.min_score_counts() == (0, 0, 0, 0)  # off again
    again = prof.sw_score_from_i8(ref)
    assert np.array_equal(again.status.cpu().numpy(), wst) and np.array_equal(again.score.cpu().numpy().view(np.uint32), ws)
