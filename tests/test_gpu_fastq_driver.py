"""GPU test of examples/zsw_driver --device-fastq: the FASTQ file read with one fread and parsed by zsw_fastq_parse_batch gives, byte
for byte, what the driver prints when it reads the file line by line on the host — on the FASTQ of tests/test_gpu_driver.py, with
--3pass --device-sam and with no other option; a malformed file ends the driver with exit status 1 and names code and record."""
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

    tmp = tmp_path_factory.mktemp("fastq_driver")
    exe = build.build_driver()
    ref = synth.reference_host(1200)
    reads = synth.reads_host(ref, 4242, 200, 100)
    reads[3] = ord("N")
    (tmp / "ref.fa").write_bytes(b">synthref test\n" + ref[:600] + b"\n" + ref[600:] + b"\n")
    text = b"".join(b"@read%d extra\n" % i + r.tobytes() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    (tmp / "reads.fq").write_bytes(text)
    lines = text.split(b"\n")
    lines[4 * 57 + 3] = lines[4 * 57 + 3][:-1] + b" "   # record 57: a blank among the qualities
    (tmp / "bad.fq").write_bytes(b"\n".join(lines))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")

    def driver(fastq, *switches):
        return subprocess.run([exe, str(tmp / "ref.fa"), str(tmp / fastq), *switches], capture_output=True, env=env, timeout=300)

    return driver


@pytest.mark.parametrize("switches", [(), ("--3pass", "--device-sam")], ids=["plain", "3pass+device-sam"])
def test_driver_device_fastq_prints_what_the_host_loop_prints(setup, switches):
    plain = setup("reads.fq", *switches)
    assert plain.returncode == 0, plain.stderr
    dev = setup("reads.fq", *switches, "--device-fastq")
    assert dev.returncode == 0, dev.stderr
    assert dev.stdout == plain.stdout and dev.stdout.count(b"\n") == 202 and b"read199\t" in dev.stdout


def test_driver_device_fastq_malformed_file(setup):
    out = setup("bad.fq", "--device-fastq")
    assert out.returncode == 1 and out.stdout == b""
    assert b"code 8" in out.stderr and b"record 57" in out.stderr
