"""GPU test of examples/zsw_driver --device-fasta / --ref-record / --fasta-reads: the reference read with one fread and parsed by
zsw_fasta_parse_batch gives, byte for byte, the SAM the driver prints with its getline loop on a one-record file; record 1 of a
two-record file gives what a file with that record alone gives; FASTA reads give the text of the Python path over the same bytes,
QUAL '*'; a malformed reference ends the driver with exit status 1 and names code and record."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

GO, GE = -10, -1


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    from zoe_amd import build, synth

    tmp = tmp_path_factory.mktemp("fasta_driver")
    exe = build.build_driver()
    ref = synth.reference_host(1200)
    other = synth.reference_host(1200)[::-1]
    reads = synth.reads_host(ref, 4242, 120, 100)
    reads[3] = ord("N")
    wrapped = b"".join(ref[i:i + 60] + b"\r\n" for i in range(0, len(ref), 60))
    (tmp / "ref.fa").write_bytes(b">synthref test\r\n" + wrapped)
    (tmp / "two.fa").write_bytes(b">other one\n" + other[:700] + b"\n" + other[700:] + b"\n>synthref test\r\n" + wrapped)
    (tmp / "bad.fa").write_bytes(b">other one\n" + other + b"\n>synthref test\r\n" + wrapped[:300] + b">" + wrapped[300:])  # a '>' behind a base: record 1
    (tmp / "reads.fq").write_bytes(b"".join(b"@read%d extra\n" % i + r.tobytes() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads)))
    fasta_reads = b"".join(b">read%d extra\n" % i + r.tobytes()[:50] + b"\n" + r.tobytes()[50:] + b"\n" for i, r in enumerate(reads))
    (tmp / "reads.fa").write_bytes(fasta_reads)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")

    def driver(reference, reads_file, *switches):
        return subprocess.run([exe, str(tmp / reference), str(tmp / reads_file), *switches], capture_output=True, env=env, timeout=300)

    driver.ref, driver.fasta_reads = ref, fasta_reads
    return driver


@pytest.mark.parametrize("switches", [(), ("--3pass", "--device-sam")], ids=["plain", "3pass+device-sam"])
def test_driver_device_fasta_prints_what_the_getline_loop_prints(setup, switches):
    plain = setup("ref.fa", "reads.fq", *switches)
    assert plain.returncode == 0, plain.stderr
    dev = setup("ref.fa", "reads.fq", *switches, "--device-fasta")
    assert dev.returncode == 0, dev.stderr
    assert dev.stdout == plain.stdout and dev.stdout.count(b"\n") == 122 and b"\tsynthref\t" in dev.stdout


def test_driver_ref_record_picks_one_record_of_many(setup):
    alone = setup("ref.fa", "reads.fq", "--device-fasta")
    second = setup("two.fa", "reads.fq", "--device-fasta", "--ref-record", "1")
    assert alone.returncode == 0 and second.returncode == 0, (alone.stderr, second.stderr)
    assert second.stdout == alone.stdout
    first = setup("two.fa", "reads.fq", "--device-fasta")
    assert first.returncode == 0 and first.stdout != alone.stdout and first.stdout.startswith(b"@HD\tVN:1.6\n@SQ\tSN:other\tLN:1200\n")
    beyond = setup("two.fa", "reads.fq", "--device-fasta", "--ref-record", "2")
    assert beyond.returncode == 1 and beyond.stdout == b"" and b"2 records" in beyond.stderr


@pytest.mark.parametrize("switches", [(), ("--device-sam",)], ids=["plain", "device-sam"])
def test_driver_fasta_reads_print_the_python_path_s_text(setup, switches):
    import zoe_amd
    from zoe_amd import records
    from zoe_amd.alignment import SeqSrc, into_local_profile

    out = setup("ref.fa", "reads.fa", "--fasta-reads", "--device-fasta", *switches)
    assert out.returncode == 0, out.stderr
    m = zoe_amd.WeightMatrix.new(zoe_amd.DNA_PROFILE_MAP, 2, -5, b"N")
    fa = records.fasta_batch_from_text(setup.fasta_reads, name_to_blank=True)
    profiles = into_local_profile(fa.as_read_batch(), m, GO, GE)
    aln = profiles.sw_align_from_i8(SeqSrc.Reference(setup.ref))
    body = profiles.to_sam_text(aln, (fa.names, fa.name_offsets), None, "synthref", 255)
    assert out.stdout == b"@HD\tVN:1.6\n@SQ\tSN:synthref\tLN:1200\n" + body
    assert body.count(b"\n") == 120 and body.count(b"\t*\tAS:i:") > 100 and b"read119\t" in body
    for extra in (("--device-fastq",), ("--from-sam", "x.sam")):
        refused = setup("ref.fa", "reads.fa", "--fasta-reads", *extra)
        assert refused.returncode == 2 and refused.stdout == b""


def test_driver_device_fasta_malformed_reference(setup):
    out = setup("bad.fa", "reads.fq", "--device-fasta", "--ref-record", "1")
    assert out.returncode == 1 and out.stdout == b""
    assert b"code 6" in out.stderr and b"record 1" in out.stderr
