"""CPU checks of the panel score pass (no GPU): the whole-reference bound of zoe_amd/csrc/zsw_seed.hpp under each member's own
parameters and index (claim W) and the panel decision built on it (seed_panel_ruled_out / seed_panel_todo: whenever a member goes
unscored, the answer — highest rank, then lowest member — is unchanged), both against the full Gotoh matrix of every read against
every member (tests/models/panel_bound.cpp), with mutants of the shipped header that the model must catch."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "models", "panel_bound.cpp")
HEADER = os.path.join(ROOT, "zoe_amd", "csrc", "zsw_seed.hpp")

_built = {}


def _build():
    if "exe" not in _built:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_panel_model_"), "panel_bound")
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, MODEL], check=True)
        _built["exe"] = exe
    return _built["exe"]


@pytest.mark.parametrize("seed", [20261018, 7])
def test_bounds_and_panel_decision_model(seed):
    """Claim W for every member and claim P over 400 panels of 2 to 6 members under the twelve scoring schemes of seed_bounds.cpp:
    near copies, identical members, members with N runs, K of 3 to 6 and the library's K on both sides of 2,048 bases; exact copies,
    copies with errors, chimeras of two members, random reads, reads of 1 to 30 bases; a quarter of the panels with an overflow
    threshold that many reads reach."""
    out = subprocess.run([_build(), "400", str(seed)], capture_output=True, text=True, timeout=900)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "panel_bound OK" in out.stdout


# One textual change each to the panel rule of zsw_seed.hpp (the target text occurs exactly once).
PANEL_MUTANTS = [
    ("the tie clause without k > p", "(u_k == s_p && k > p)", "(u_k == s_p)"),
    ("<= in place of <", "    return u_k < s_p || (u_k == s_p", "    return u_k <= s_p || (u_k == s_p"),
    ("settling when the status is not SOME", "    if (!some_p || u_k < 0) return false;", "    if (u_k < 0) return false;"),
]


@pytest.mark.parametrize("name,old,new", PANEL_MUTANTS, ids=[m[0] for m in PANEL_MUTANTS])
def test_panel_model_kills_mutants_of_the_shipped_header(tmp_path, name, old, new):
    """The model has teeth: each weakening of the rule, compiled into the model in place of the shipped header, makes it report a
    violated claim P at the committed iteration count."""
    src = open(HEADER).read()
    assert src.count(old) == 1, f"mutation target of {name!r} is not unique in zsw_seed.hpp"
    header = tmp_path / "zsw_seed.hpp"
    header.write_text(src.replace(old, new))
    exe = str(tmp_path / "panel_bound")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", f'-DZSW_SEED_HEADER="{header}"', "-o", exe, MODEL], check=True)
    out = subprocess.run([exe, "400", "20261018"], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode != 0, f"mutant survived: {name}\n{out.stdout}"
    assert "claim P violated" in out.stdout
    assert "panel_bound OK" not in out.stdout


def test_report_mode_prints_settled_share_and_members_scored_per_divergence_rate():
    """The table of DESIGN 4.13: every exact copy is settled after one score, every random read is scored against all 8 members;
    at 1 % + 0.1 % fewer than 8 members are scored per read on both panels (what tests/test_gpu_panel.py expects of the counters)."""
    out = subprocess.run([_build(), "report", "200", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    tables = out.stdout.split("panel of ")[1:]
    assert len(tables) == 2
    for t in tables:
        rows = {line[:28].strip(): line[28:].split() for line in t.splitlines()[2:]}
        assert rows["0.0 % + 0.0 %"][1:] == ["100.0", "1.00"]
        assert rows["random reads"][1:] == ["0.0", "8.00"]
        assert float(rows["1.0 % + 0.1 %"][2]) < 2.0


def test_model_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the model as a stand-alone program built with -fsanitize=address,undefined: the shipped header's sweeps, look-ups and the
    64-bit lists stay inside their arrays and shift widths"""
    exe = str(tmp_path / "panel_bound_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, MODEL],
                   check=True)
    out = subprocess.run([exe, "96", "11"], capture_output=True, text=True, timeout=900)
    print(out.stdout[-1000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "panel_bound OK" in out.stdout and "runtime error" not in out.stderr
