"""CPU check of diag_walk_is_interior (zoe_amd/csrc/zsw_seed_diag.hpp), the predicate by which a wavefront of the diagonal first tier
takes the column loop without edge masks, no GPU: tests/models/seed_diag_interior.cpp, also built with the address and
undefined-behaviour sanitizers and run on its own."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "models", "seed_diag_interior.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request):
    exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), "seed_diag_interior_" + request.param)
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC], check=True)
    return exe


def test_the_predicate_implies_all_ones_words_and_is_tight(program):
    """R in {40, 300, 2000}, L in {24, 25, 150, 255}, dtmin in [-L - 20, R + 20], dtmax - dtmin in {0, 1}: wherever the predicate
    holds the five edge words are all-ones in every executed column of every group, wherever it does not one of them lacks a bit; it
    is false on either side of every reference and true from first band row 1 to first row below the band R - 1."""
    out = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seed_diag_interior OK" in out.stdout
    m = re.search(r"interior walks at R 2000, L 150: (\d+) of (\d+) anchors", out.stdout)
    # anchors 9 .. 2000 - 1 - 6 - 150 of 0 .. 1850
    assert m and (int(m.group(1)), int(m.group(2))) == (1835, 1851), out.stdout
    print(out.stdout)


def test_the_narrow_band_of_the_model_is_the_kernels():
    with open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_score_seed.hpp")) as f:
        text = f.read()
    wu = int(re.search(r"SEED_NARROW_WU = (\d+)", text).group(1))
    wd = int(re.search(r"SEED_NARROW_WD = (\d+)", text).group(1))
    with open(SRC) as f:
        model = f.read()
    assert f"WU = {wu}, WD = {wd}" in model
