"""CPU check of the co-scheduled full pass's host side (zoe_amd/csrc/zsw_handback.hpp: handback_coschedule, handback_blocks,
coschedule_role, handback_block_range), no GPU: tests/models/coschedule_plan.cpp. In a score-only call of two band tiers the reads
the seed kernel hands back are scored inside the first tier's launch: the first blocks of the grid own the pairs of the list, the
blocks behind them are the tier's. A pair no block owns is a read nobody scores; a pair two blocks own is scored twice."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_exe = {}


def _build():
    if "coschedule_plan" not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), "coschedule_plan")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "models", "coschedule_plan.cpp")], check=True)
        _exe["coschedule_plan"] = exe
    return _exe["coschedule_plan"]


def test_every_pair_of_the_list_is_owned_by_exactly_one_handback_block():
    """Classes of 1 .. 10,000,000 reads; list lengths 0, 1, 2, 127, 128, 129 (a block of the four-lane configurations holds 64
    pairs = 128 reads) and n_items, for every lane count: the roles partition the grid, the hand-back blocks own the list's pairs in
    order, each once, none beyond the list — and the ranges are those score_kernel_v2's own index arithmetic gives."""
    args = []
    for n in (1, 2, 127, 128, 129, 257, 4097, 200000, 10000000):
        for count in (0, 1, 2, 127, 128, 129, n):
            if count <= n:
                args += [str(n), str(count)]
    out = subprocess.run([_build(), "split"] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    checks, violations = (int(v) for v in re.fullmatch(r"coschedule_plan split: (\d+) checks, (\d+) violations", lines[-1]).groups())
    assert checks == len(args) // 2 * 5 * 4
    assert violations == len(lines) - 1 == 0, lines[:10]


def test_the_decision_holds_for_score_only_two_tier_diagonal_four_lane_calls_alone():
    """mode 0 .. 3, one or two tiers, strips or diagonals in the first, G = 4 .. 64, ZSW_OPTION_MIN_SCORE, row chunks, hand-backs the
    caller settles itself, ZSW_DEBUG_SEED_NO_COSCHEDULE: of the 1,280 cases exactly one is co-scheduled."""
    out = subprocess.run([_build(), "decide"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [tuple(int(v) for v in re.fullmatch(r"DECIDE (\d) (\d) (\d) (\d+) (\d) (\d) (\d) (\d) -> (\d)", ln).groups()) for ln in out.stdout.splitlines()]
    assert len(rows) == len(set(r[:-1] for r in rows)) == 4 * 5 * 64
    yes = [r[:-1] for r in rows if r[-1]]
    #        mode tiers diagonal G mins chunks skip disabled
    assert yes == [(0, 1, 1, 4, 0, 0, 0, 0)], yes
