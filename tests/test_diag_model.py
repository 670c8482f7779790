"""CPU check of the diagonal first tier (seed_diag_kernel, zoe_amd/csrc/zsw_score_band.hip), no GPU: the banded pass with strips
of ONE column, which the strip model's own generator (tests/test_align_models.py: strips of 5-64 columns) never draws."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_exe = {}


def _build():
    if "seed_diag" not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), "seed_diag")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "models", "seed_diag.cpp")], check=True)
        _exe["seed_diag"] = exe
    return _exe["seed_diag"]


@pytest.mark.parametrize("seed", [20261019, 5])
def test_one_column_strips_bounds_model_and_the_kernel_s_twin(seed):
    """tests/models/seed_diag.cpp: (1) the checks of seed_band.cpp at C = 1, for every read whether accepted or not — every cell
    of the band holds a bound >= its true H, every cell outside is <= a(c) / b(c) and <= oa / ob, every class of outside paths stays
    under its own bound programme, an accepted read has the true score (and, ends tag, the true first row and column) — over the
    eleven schemes, lane partners whose anchors lie up to the kernel's slack (1) and one beyond it apart, partners of different
    lengths, reads over both ends of the reference, every structured case of adversarial_reads.hpp; (2) a plain-integer twin of
    the kernel's walk (a register per diagonal, a column per step, the neutral table entry outside the reference, the column masks
    of a 16-column group, the spare diagonal of a pair with one anchor) must return the strip walk's (maximum, oa, ob) at C = 1 on
    every read; (3) zsw_seed_diag.hpp's seed_free_bits equals seed_exit_is_free column by column. The per-class check costs
    O(columns) full matrices per read at C = 1, hence 16 references x 72 reads per seed."""
    out = subprocess.run([_build(), "16", str(seed)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "seed_diag OK" in out.stdout
