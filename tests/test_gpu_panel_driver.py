"""GPU test of examples/zsw_driver --panel: on a 3-record FASTA and 200 reads the driver prints the text defined by equivalence —
today's driver run once per record (--device-fasta --ref-record K --3pass); per read the line of the run of its best record (the
highest AS:i, ties to the lowest record, a read unmapped everywhere from record 0); the header lines of the three runs in record
order, a line that repeats in every run once. The flag combinations --panel refuses exit with status 2 and a message."""
import os
import subprocess

import numpy as np
import pytest

from conftest import stable_seed

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    from zoe_amd import build

    tmp = tmp_path_factory.mktemp("panel_driver")
    exe = build.build_driver()
    rng = np.random.default_rng(stable_seed("panel-driver"))
    members = [ACGT[rng.integers(0, 4, L)] for L in (600, 1500, 2100)]
    members.append(members[1].copy())  # a fourth record identical to the second: its reads tie, and go to the second
    reads = []
    for i in range(200):
        if i % 10 == 9:
            q = ACGT[rng.integers(0, 4, 100)] if i % 20 == 9 else np.full(100, ord("N"), dtype=np.uint8)  # random reads, and reads unmapped everywhere
        else:
            m = members[i % 3]
            s = int(rng.integers(0, len(m) - 110))
            q = m[s:s + 110].copy()
            hit = rng.random(110) < 0.04
            q[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
            if i % 7 == 0:
                q = np.delete(q, 50)
            q = q[:100]
        reads.append(q.tobytes())
    fasta = b"".join(b">seg%d subtype %d\n" % (k, k) + b"\n".join(m.tobytes()[i:i + 70] for i in range(0, len(m), 70)) + b"\n" for k, m in enumerate(members))
    (tmp / "panel.fa").write_bytes(fasta)
    (tmp / "reads.fq").write_bytes(b"".join(b"@read%d extra\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads)))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")

    def driver(*switches):
        return subprocess.run([exe, str(tmp / "panel.fa"), str(tmp / "reads.fq"), *switches], capture_output=True, env=env, timeout=300)

    driver.n_members, driver.n_reads = len(members), len(reads)
    return driver


def _score(line: bytes) -> int:
    fields = line.split(b"\t")
    if int(fields[1]) & 4:
        return 0
    return int([f for f in fields if f.startswith(b"AS:i:")][0][5:])


@pytest.mark.parametrize("extra", [(), ("--device-fastq",)], ids=["getline reads", "device-fastq"])
def test_driver_panel_prints_the_text_defined_by_the_per_record_runs(setup, extra):
    K, n = setup.n_members, setup.n_reads
    runs = []
    for k in range(K):
        out = setup("--device-fasta", "--ref-record", str(k), "--3pass", *extra)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines(keepends=True)
        runs.append(([x for x in lines if x.startswith(b"@")], [x for x in lines if not x.startswith(b"@")]))
        assert len(runs[-1][1]) == n
    header, seen = [], set()
    for k in range(K):
        for line in runs[k][0]:
            if all(line in r[0] for r in runs):
                if line in seen:
                    continue
                seen.add(line)
            header.append(line)
    body, best_of = [], []
    for i in range(n):
        scores = [_score(runs[k][1][i]) for k in range(K)]
        best = int(np.argmax(scores))  # the first maximum: ties go to the lowest record; all zero: record 0
        best_of.append(best)
        body.append(runs[best][1][i])
    want = b"".join(header + body)
    assert set(best_of) == {0, 1, 2} and best_of.count(0) > 40  # (record 3 never wins: it ties with record 1)
    assert want.count(b"\t4\t*\t") >= 10 and want.startswith(b"@HD\tVN:1.6\n@SQ\tSN:seg0\tLN:600\n@SQ\tSN:seg1\tLN:1500\n@SQ\tSN:seg2\tLN:2100\n@SQ\tSN:seg3\tLN:1500\n")
    got = setup("--panel", *extra)
    assert got.returncode == 0, got.stderr
    assert got.stdout == want


@pytest.mark.parametrize("extra", [("--both-strands",), ("--from-sam", "x.sam"), ("--consensus", "c.fa"), ("--score-only",)])
def test_driver_panel_refuses_what_it_does_not_cover(setup, extra):
    out = setup("--panel", *extra)
    assert out.returncode == 2 and out.stdout == b""
    assert b"--panel" in out.stderr and extra[0].encode() in out.stderr
