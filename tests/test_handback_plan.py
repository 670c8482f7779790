"""CPU check of the launch plan for the reads the seeded pass hands back (zoe_amd/csrc/zsw_handback.hpp, compiled by seed_items of
zsw_score.hip), no GPU: tests/models/handback_plan.cpp. The list's length exists only on the device; whatever it is, exactly one of
the gated score_kernel_v2 launches must take it — a count that no gate holds leaves its reads unscored."""
import os
import re
import subprocess
import tempfile

import strip_edge_reads as ser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_exe = {}


def _build():
    if "handback_plan" not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), "handback_plan")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "models", "handback_plan.cpp")], check=True)
        _exe["handback_plan"] = exe
    return _exe["handback_plan"]


def _run(rule):
    with open(os.path.join(ROOT, "zoe_amd", "csrc", "zsw_score.hip")) as f:
        n_ascending = int(re.search(r"constexpr int N_ASCENDING_CFGS = (\d+);", f.read()).group(1))
    cfgs = ser.strip_configs()
    assert n_ascending == 20 and len(cfgs) == 21
    out = subprocess.run([_build(), rule, str(n_ascending)] + [f"{g},{c}" for g, c in cfgs], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    checks, violations = (int(v) for v in re.fullmatch(rf"handback_plan {rule}: (\d+) checks, (\d+) violations", lines[-1]).groups())
    assert violations == len(lines) - 1
    return checks, lines[:-1]


def test_exactly_one_gated_launch_takes_every_count():
    """Every read length 24 .. 2,432 in its first-fit configuration, n_items in {1, 2, 1,023, 49,151 .. 49,153, 327,679 .. 327,681,
    1,000,000}, every count in {1, n - 1, n, 49,151 .. 49,153, 327,679 .. 327,681} up to n_items, and every set of lane counts whose
    score tables cannot be built (the range then falls to a later launch): one launch with lo <= count < hi, its grid covers the
    count, its G * C holds the length."""
    checks, violations = _run("plan")
    assert checks > 2409 * 10 * 32 * 3
    assert not violations, violations[:10]


def test_the_invariant_tells_the_strict_comparison_apart():
    """The loop as it was before the plan was a function of its own launched a range only if n_items > lo. With n_items = count =
    49,152 the gate [0, 49,152) of the short-list configuration is launched and does not hold the count, and the class's own
    configuration behind it, gate [49,152, ...), was not launched: nothing scored the list. That is so for every length whose
    16,384-read configuration differs from the first fit (24 .. 304 bases except 161 .. 176, where both are (8,22)) unless that configuration's tables cannot be built; the
    128 k configuration is the first fit for every length, so the cut at 327,680 never starts a gate. The check above must see this."""
    _, violations = _run("strict")
    got = set()
    for v in violations:
        m = re.fullmatch(r"VIOLATION len (\d+) n (\d+) count (\d+) fail (\d+) taken (\d+) fits (\d+)", v)
        assert m, v
        L, n, count, fail, taken, fits = (int(x) for x in m.groups())
        assert (n, count, taken) == (49152, 49152, 0), v
        if fail == 0:
            got.add(L)
    cfgs = ser.strip_configs()

    def for_batch(L, n):  # score_config_for_batch
        best, pick = 0.0, None
        for G, C in cfgs:
            cost = (7.5 * C + 25.0) * max(2048.0, ((n + 1) // 2) * G / 64.0)
            if G * C >= L and (pick is None or cost < best * 0.97):
                best, pick = cost, (G, C)
        return pick

    first_fit = lambda L: next((G, C) for G, C in cfgs[:20] if G * C >= L)
    want = {L for L in range(24, 2433) if for_batch(L, 16384)[0] != first_fit(L)[0]}
    assert all(for_batch(L, 131072)[0] == first_fit(L)[0] for L in range(24, 2433))
    assert got == want, sorted(got ^ want)[:10]
    assert (min(got), max(got), len(got)) == (24, 304, 265) and set(range(24, 305)) - got == set(range(161, 177))  # (8,22) either way
