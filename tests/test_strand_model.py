"""CPU checks of the strand-aware score pass (no GPU): the whole-reference bound of zoe_amd/csrc/zsw_seed.hpp (claim W: no local
alignment of a sequence against the reference scores more than seed_whole_bound().u) and the strand decision built on it, both
against the full Gotoh matrix for the two orientations of every read (tests/models/strand_bound.cpp), with mutants of the
shipped header that the model must catch."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "models", "strand_bound.cpp")
HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_seed.hpp")

_built = {}


def _build():
    if "exe" not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_strand_model_"), "strand_bound")
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, MODEL], check=True)
        _built["exe"] = exe
    return _built["exe"]


@pytest.mark.parametrize("seed", [20261018, 7])
def test_whole_reference_bound_and_strand_decision_model(seed):
    """Claim W for both orientations of every read and claim R (a settled read's answer is the contract's) over 400 references x
    84 reads: twelve scoring schemes, K of 3 to 6, inverted repeats, palindromes, N runs, chimeras of both strands, reads of
    1 to 30 bases, and the structured cases whose columns between two k-mers have no potential."""
    out = subprocess.run([_build(), "400", str(seed)], capture_output=True, text=True, timeout=900)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "strand_bound OK" in out.stdout


# One textual change each to the new functions of zsw_seed.hpp (the target text occurs exactly once).
STRAND_MUTANTS = [
    ("unusable k-mers are charged", "        const bool in = j < s.m && s.usable[j];", "        const bool in = j < s.m;"),
    ("t_all - lambda * count instead of the span maximum", "    out.u = seed_span_bound(s.m, s.pot_lo, s.pot_hi, s.t_all, set, s.lam);",
     "    { int cnt = 0; for (int j = 0; j < s.m; ++j) cnt += set[j] ? 1 : 0; out.u = s.t_all - s.lam * cnt; if (out.u < 0) out.u = 0; }"),
    ("the run >= lambda rule for the columns in front of a k-mer is off", "        bool ok = j == 0 || run >= s->lam;", "        bool ok = true;"),
]


@pytest.mark.parametrize("name,old,new", STRAND_MUTANTS, ids=[m[0] for m in STRAND_MUTANTS])
def test_strand_model_kills_mutants_of_the_shipped_header(tmp_path, name, old, new):
    """The model has teeth: each weakening of seed_whole_bound, compiled into the model in place of the shipped header, makes it
    report a violated claim at the committed iteration count (the comparison of the sweep with seed_read's is compiled out, so that
    the claims themselves have to catch it)."""
    src = open(HEADER).read()
    assert src.count(old) == 1, f"mutation target of {name!r} is not unique in zsw_seed.hpp"
    header = tmp_path / "zsw_seed.hpp"
    header.write_text(src.replace(old, new))
    exe = str(tmp_path / "strand_bound")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", f'-DZSW_SEED_HEADER="{header}"', "-DZSW_STRAND_NO_TWIN_CHECK", "-o", exe, MODEL], check=True)
    out = subprocess.run([exe, "400", "20261018"], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode != 0, f"mutant survived: {name}\n{out.stdout}"
    assert "claim W violated" in out.stdout or "claim R violated" in out.stdout
    assert "strand_bound OK" not in out.stdout


def test_report_mode_prints_the_settled_share_per_divergence_rate():
    """The table of DESIGN 4.6: every exact copy is settled, no random read is."""
    out = subprocess.run([_build(), "report", "200", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {line[:28].strip(): line[28:].split() for line in out.stdout.splitlines()[2:]}
    assert rows["0.0 % + 0.0 %"][1] == "100.0"
    assert rows["random reads"][1] == "0.0"
