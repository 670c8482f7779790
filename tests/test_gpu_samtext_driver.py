"""GPU test of examples/zsw_driver --from-sam on a file the driver itself wrote: with --device-sam it writes that file again byte
for byte (forward and --both-strands runs, plain and with --nm --verbose-cigar), without --device-sam the host loop prints the same,
with --consensus it gives the FASTA of the aligning run, and a malformed file ends the driver with exit status 1 naming the line."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    from zoe_amd import build, synth

    tmp = tmp_path_factory.mktemp("samtext_driver")
    exe = build.build_driver()
    ref = synth.reference_host(1200)
    reads = synth.reads_host(ref, 4242, 200, 100)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = [r.tobytes() if i % 2 == 0 else r.tobytes().translate(comp)[::-1] for i, r in enumerate(reads)]  # every other read from the reverse strand
    seqs[3] = b"N" * 100
    (tmp / "ref.fa").write_bytes(b">synthref test\n" + ref[:600] + b"\n" + ref[600:] + b"\n")
    (tmp / "reads.fq").write_bytes(b"".join(b"@read%d extra\n" % i + s + b"\n+\n" + bytes(33 + (i + k) % 90 for k in range(len(s))) + b"\n" for i, s in enumerate(seqs)))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")

    def driver(reads_arg, *switches):
        return subprocess.run([exe, str(tmp / "ref.fa"), reads_arg if reads_arg == "-" else str(tmp / reads_arg), *switches], capture_output=True, env=env, timeout=300)

    return driver, tmp


@pytest.mark.parametrize("align", [("--3pass",), ("--both-strands",)], ids=["3pass", "both-strands"])
def test_driver_from_sam_writes_the_file_it_read(setup, align):
    driver, tmp = setup
    first = driver("reads.fq", *align, "--device-sam", "--consensus", str(tmp / "first.fa"))
    assert first.returncode == 0, first.stderr
    assert first.stdout.count(b"\n") == 202 and b"\t4\t*\t0\t0\t*\t" in first.stdout and (align == ("--3pass",) or b"\t16\tsynthref\t" in first.stdout)
    sam = tmp / "first.sam"
    sam.write_bytes(first.stdout)
    again = driver("-", "--from-sam", str(sam), "--device-sam", "--consensus", str(tmp / "again.fa"))
    assert again.returncode == 0, again.stderr
    assert again.stdout == first.stdout                                             # header and body, byte for byte
    assert (tmp / "again.fa").read_bytes() == (tmp / "first.fa").read_bytes()       # the same consensus as the aligning run
    host = driver("-", "--from-sam", str(sam))                                      # the host loop prints the same lines
    assert host.returncode == 0 and host.stdout == first.stdout
    want = driver("reads.fq", *align, "--device-sam", "--nm", "--verbose-cigar")    # the annotation runs on the file's records
    got = driver("-", "--from-sam", str(sam), "--device-sam", "--nm", "--verbose-cigar")
    assert want.returncode == 0 and got.returncode == 0, (want.stderr, got.stderr)
    assert got.stdout == want.stdout and b"\tNM:i:" in got.stdout and b"=" in got.stdout


def test_driver_from_sam_malformed_file_and_arguments(setup):
    driver, tmp = setup
    first = driver("reads.fq", "--3pass", "--device-sam")
    assert first.returncode == 0, first.stderr
    lines = first.stdout.split(b"\n")
    fields = lines[59].split(b"\t")  # two header lines in front: this is line 60 of the file
    fields[4] = b"256"
    lines[59] = b"\t".join(fields)
    (tmp / "bad.sam").write_bytes(b"\n".join(lines))
    out = driver("-", "--from-sam", str(tmp / "bad.sam"), "--device-sam")
    assert out.returncode == 1 and out.stdout == b""
    assert b"line 60" in out.stderr and b"mapq" in out.stderr and b"code 5" in out.stderr
    assert driver("-", "--from-sam", str(tmp / "bad.sam"), "--3pass").returncode == 2
    assert driver("-", "--from-sam", str(tmp / "missing.sam")).returncode == 1
