"""GPU test of examples/zsw_driver --consensus FILE: the one-record FASTA it writes beside the SAM output equals the Python path's
(pileup() of the profile class, plurality_acgtn with the reference as fallback) on the driver's test FASTQ, under the default call,
--3pass and --both-strands; the SAM output itself is what it is without the switch."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GO, GE = -10, -1


@pytest.mark.parametrize("mode", ["", "--3pass", "--both-strands"])
def test_driver_consensus(tmp_path, mode):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd as za
    from zoe_amd import build, synth

    exe = build.build_driver()
    true_ref = synth.reference_host(1200)
    reads = synth.reads_host(true_ref, 4242, 300, 100)
    reads[3] = ord("N")
    reads = [r.tobytes() for r in reads]
    if mode == "--both-strands":
        rc = bytes.maketrans(b"ACGT", b"TGCA")
        reads = [r.translate(rc)[::-1] if k % 3 == 0 else r for k, r in enumerate(reads)]
    ref = bytearray(true_ref)
    for k in range(40, 1160, 61):  # the reads come from true_ref: the consensus repairs these where reads cover them
        ref[k] = ord("ACGT"["ACGT".index(chr(ref[k])) ^ 1])
    PAD = 40
    ref = b"A" * PAD + bytes(ref) + b"C" * PAD  # ends no read comes from
    (tmp_path / "ref.fa").write_bytes(b">synthref test\n" + ref + b"\n")
    with open(tmp_path / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d extra\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + e.get("LD_LIBRARY_PATH", "")
    switches = [mode] if mode else []

    def driver(*extra):
        out = subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), *switches, *extra], capture_output=True, text=True, env=e, timeout=300)
        assert out.returncode == 0, out.stderr
        return out.stdout

    plain = driver()
    fa = tmp_path / "consensus.fa"
    assert driver("--consensus", str(fa)) == plain
    lines = fa.read_bytes().split(b"\n")
    assert lines[0] == b">synthref_consensus" and lines[2:] == [b""]
    got = lines[1]

    m = za.WeightMatrix.new(za.DNA_PROFILE_MAP, 2, -5, b"N")
    prof = za.into_local_profile(reads, m, GO, GE)
    src = za.SeqSrc.Reference(ref)
    aln = {"": prof.sw_align_from_i8, "--3pass": prof.sw_align_from_i8_3pass, "--both-strands": prof.sw_align_strands_from_i8_3pass}[mode](src)
    counts = prof.pileup(aln, src)
    want = za.plurality_acgtn(counts, fallback=ref).cpu().numpy().tobytes()
    assert got == want
    covered = counts.cpu().numpy()[:, :5].sum(axis=1) > 0
    assert covered.sum() > 1000 and not covered.all()                        # the uncovered ends keep the reference's bases
    assert all(got[k] == ref[k] for k in np.nonzero(~covered)[0])
    repaired = [k for k in range(40, 1160, 61) if covered[PAD + k]]
    assert len(repaired) >= 10 and sum(1 for k in repaired if got[PAD + k] == true_ref[k]) >= len(repaired) - 2
    out = subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), "--score-only", "--consensus", str(fa)], capture_output=True, text=True, env=e, timeout=300)
    assert out.returncode == 2 and "--consensus" in out.stderr
