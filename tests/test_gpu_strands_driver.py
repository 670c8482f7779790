"""examples/zsw_driver.cpp --both-strands: a FASTQ of both strands in, SAM out with flag 16, SEQ reverse complemented and QUAL
reversed for the reads answered by their reverse complement; without the flag the driver writes what it always wrote."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_strands import mixed_strand_reads, rc

pytestmark = pytest.mark.gpu


def _sam_line(name, flag, ref_name, aln, i, seq, qual):
    r = aln.records[i]
    return "\t".join([name, str(flag), ref_name, str(int(r["ref_start"]) + 1), "255", aln.cigar(i), "*", "0", "0", seq, qual, f"AS:i:{int(r['score'])}"])


def test_driver_both_strands(tmp_path, oracle):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd as za
    from zoe_amd import build, synth

    exe = build.build_driver()
    ref = synth.reference_host(1200)
    reads = mixed_strand_reads(ref, 120, 100, 77, rates=(0.01, 0.06), random_share=0.05)
    rng = np.random.default_rng(7)
    quals = ["".join(chr(int(x)) for x in rng.integers(35, 74, len(q))) for q in reads]  # '#'..'I' (the driver reads four lines per record, so a quality line may start with '@')
    (tmp_path / "ref.fa").write_bytes(b">synthref test\n" + ref[:600] + b"\n" + ref[600:] + b"\n")
    with open(tmp_path / "reads.fq", "wb") as f:
        for i, q in enumerate(reads):
            f.write(b"@read%d extra\n" % i + q + b"\n+\n" + quals[i].encode() + b"\n")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    run = lambda *flags: subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), *flags], capture_output=True, text=True, env=env, timeout=300)
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    prof = za.LocalProfilesBatch.new_with_w256(reads, m, -10, -1)
    header = f"@HD\tVN:1.6\n@SQ\tSN:synthref\tLN:{len(ref)}\n"

    # with the flag: flag, POS and CIGAR of the Python mirror's strand call, SEQ and QUAL as aligned
    both = prof.sw_align_strands_from_i8_3pass(za.SeqSrc.Reference(ref))
    sc = oracle.dna_scoring(2, -5, b"N", -10, -1)
    want = []
    for i, q in enumerate(reads):
        sf = oracle.cascade_score(8, 256, sc, q, ref)
        sr = oracle.cascade_score(8, 256, sc, rc(q), ref)
        strand = int(sr[0] == 0 and (sf[0] != 0 or sr[1] > sf[1]))
        assert int(both.strand[i]) == strand, i
        if int(both.status[i]) == 0:
            want.append(_sam_line(f"read{i}", 16 * strand, "synthref", both, i, (rc(q) if strand else q).decode(), quals[i][::-1] if strand else quals[i]))
        else:
            want.append(f"read{i}\t4\t*\t0\t0\t*\t*\t0\t0\t{q.decode()}\t{quals[i]}")
    assert 40 < int(both.strand.sum()) < 80
    out = run("--both-strands")
    assert out.returncode == 0, out.stderr
    assert out.stdout == header + "\n".join(want) + "\n"

    # without it: byte for byte the SAM the driver has always written (flag 0, the reads and qualities as given)
    fwd = prof.sw_align_from_i8(za.SeqSrc.Reference(ref))
    plain = [_sam_line(f"read{i}", 0, "synthref", fwd, i, q.decode(), quals[i]) if int(fwd.status[i]) == 0 else
             f"read{i}\t4\t*\t0\t0\t*\t*\t0\t0\t{q.decode()}\t{quals[i]}" for i, q in enumerate(reads)]
    out = run()
    assert out.returncode == 0, out.stderr
    assert out.stdout == header + "\n".join(plain) + "\n"
