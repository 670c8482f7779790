"""CPU check of the two-phase seed kernel's arithmetic (zoe_amd/csrc/zsw_seed_packed.hpp: seed_pack_window, seed_pack8 and
seed_read_packed, what seed_packed_kernel runs) against seed_read, no GPU: tests/models/seed_packed.cpp. On the GPU:
tests/test_gpu_seed_packed.py."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_exe = {}


def _build():
    if "seed_packed" not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), "seed_packed")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "models", "seed_packed.cpp")], check=True)
        _exe["seed_packed"] = exe
    return _exe["seed_packed"]


def _constant(name, header):
    with open(os.path.join(ROOT, "zoe_amd", "csrc", header)) as f:
        return int(re.search(r"constexpr \w+ " + name + r" = (\d+);", f.read()).group(1))


def test_packed_rows_and_every_field_equal_seed_read():
    """Every read length SEED_MIN_LEN .. SEED_PACKED_MAX_LEN, K = 8 .. 12, spacer 2 .. 4, both orientations, three matrices (N with
    potential 0 and 1, permuted codes with a good residue below maxw) and references of 60, 300 and 2,000 bases; 24 reads per layout in
    a buffer of exactly their bytes — copies with substitutions, with one N, runs of N and bytes outside the alphabet anywhere and
    just before, inside and just behind a sampled k-mer, unrelated reads: the residue codes are what seed_kernel packs, the flag is set
    exactly for the reads with a column that is not plain, and seed_read_packed returns every field of seed_read, u_whole included."""
    lo, hi = _constant("SEED_MIN_LEN", "zsw_score_seed.hpp"), _constant("SEED_PACKED_MAX_LEN", "zsw_seed_packed.hpp")
    assert (lo, hi) == (24, 160)
    assert hi == _constant("SEED_STAGE_LEN", "../csrc/zsw_score_seed.hip")
    out = subprocess.run([_build(), str(lo), str(hi), "24", "20261019"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seed_packed OK" in out.stdout
    n = int(re.match(r"(\d+) reads", out.stdout).group(1))
    assert n > 250000, out.stdout
