"""CPU checks of ZSW_OPTION_MIN_SCORE (no GPU): the two upper bounds that settle a read as "below the caller's minimum" — claim
W's bound as seed_read<true> returns it, and seed_band_upper over what a band walk leaves — and the decision built on them, against
the full Gotoh matrix (tests/models/min_score.cpp, which compiles zoe_amd/csrc/zsw_seed.hpp and, in their library mode, the models
strand_bound.cpp and seed_band.cpp that hold the claims the bounds come from), with mutants of the shipped header that the model
must catch."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "models")
HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_seed.hpp")
SOURCES = ("min_score.cpp", "strand_bound.cpp", "seed_band.cpp", "adversarial_reads.hpp")

_built = {}


def _compile(tree: str) -> str:
    """the model of the tree `tree` (tests/models + zoe_amd/csrc/zsw_seed.hpp, by the model's relative include)"""
    exe = os.path.join(tree, "min_score")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-o", exe,
                    os.path.join(tree, "tests", "models", "min_score.cpp")], check=True)
    return exe


def _tree(base: str, header_text: str) -> str:
    os.makedirs(os.path.join(base, "tests", "models"))
    os.makedirs(os.path.join(base, "zoe_amd", "csrc"))
    for f in SOURCES:
        shutil.copy(os.path.join(MODELS, f), os.path.join(base, "tests", "models", f))
    with open(os.path.join(base, "zoe_amd", "csrc", "zsw_seed.hpp"), "w") as f:
        f.write(header_text)
    return base


def _build():
    if "exe" not in _built:
        _built["exe"] = _compile(_tree(os.path.join(tempfile.mkdtemp(prefix="zsw_min_score_model_"), "t"), open(HEADER).read()))
    return _built["exe"]


@pytest.mark.parametrize("seed", [20261019, 11])
def test_bounds_and_decision_rule_against_the_full_matrix(seed):
    """400 references x (60 reads of strand_bound.cpp's classes + 12 of its structured cases), its twelve schemes: the whole-read
    bound of seed_read equals seed_whole_bound().u and bounds the matrix; for the eleven schemes of seed_band.cpp every anchored read
    is walked in strips of 5 - 32 columns, accepted or not, in both taggings, and seed_band_upper bounds every cell; the contract's
    answer from the matrix equals "settled by the bound, else exact" for T in {1, true, true + 1, bound, bound + 1, thr, thr + 1}."""
    out = subprocess.run([_build(), "400", str(seed)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "min_score OK" in out.stdout


# One textual change each to the new functions of zsw_seed.hpp (the target text occurs exactly once).
MUTANTS = [
    ("floor instead of ceiling in seed_band_upper", "    const int in = (int)((b2 + 1u) >> 1);", "    const int in = (int)(b2 >> 1);"),
    ("ob dropped from seed_band_upper", "    const int out = oa > ob ? oa : ob;", "    const int out = oa;"),
    ("<= T instead of < T in seed_below_min", "{ return bound < t; }", "{ return bound <= t; }"),
]


@pytest.mark.parametrize("name,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_model_kills_mutants_of_the_shipped_header(tmp_path, name, old, new):
    """The model has teeth: each weakening, compiled into the model in place of the shipped header, makes it report a violated
    claim at the committed iteration count."""
    src = open(HEADER).read()
    assert src.count(old) == 1, f"mutation target of {name!r} is not unique in zsw_seed.hpp"
    exe = _compile(_tree(str(tmp_path / "t"), src.replace(old, new)))
    out = subprocess.run([exe, "400", "20261019"], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode != 0, f"mutant survived: {name}\n{out.stdout}"
    assert "band bound violated" in out.stdout or "decision rule violated" in out.stdout
    assert "min_score OK" not in out.stdout


def test_report_mode_prints_which_route_settles_the_reads_below_the_minimum():
    """The table of DESIGN 4.1e: at T = 225 every random read is below T and the whole-read bound settles all of them; no exact copy
    is below any T of the table."""
    out = subprocess.run([_build(), "report", "150", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {line[:22].strip(): [c.split() for c in line[22:].split("|")[1:]] for line in out.stdout.splitlines()[3:]}
    assert len(rows) == 8, out.stdout
    t225 = rows["random reads"][2]
    assert float(t225[0]) == 100.0 and float(t225[2]) == 100.0, t225
    assert all(float(c[0]) == 0.0 for c in rows["0.0 % + 0.0 % indels"])
