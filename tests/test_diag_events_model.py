"""CPU check of the loop-free group events of the diagonal first tier (zoe_amd/csrc/zsw_seed_diag.hpp: seed_group_patterns and
seed_group_pick, what seed_diag_kernel derives once per group of sixteen columns), no GPU: tests/models/seed_diag_events.cpp."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_exe = {}


def _build():
    if "seed_diag_events" not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), "seed_diag_events")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "models", "seed_diag_events.cpp")], check=True)
        _exe["seed_diag_events"] = exe
    return _exe["seed_diag_events"]


def _constant(name):
    with open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_score_seed.hpp")) as f:
        return int(re.search(r"constexpr \w+ " + name + r" = (\d+);", f.read()).group(1))


def test_group_events_equal_the_loops_for_every_layout():
    """Every read length SEED_MIN_LEN .. SEED_DIAG_MAX_LEN, K = 8 .. 12, spacer 2 .. 4, every group start, the masks 0, all-ones,
    every single bit and 300 random ones per layout: the masked start / end / inside / free bits equal seed_strip_events and
    seed_free_bits bit for bit, no fourth k-mer touches a group, the territory bits equal seed_exit_is_free column by column."""
    lo, hi = _constant("SEED_MIN_LEN"), _constant("SEED_DIAG_MAX_LEN")
    assert (lo, hi) == (24, 255)
    out = subprocess.run([_build(), str(lo), str(hi), "300", "20261019"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seed_diag_events OK" in out.stdout
